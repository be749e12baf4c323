"""Thin Python face of the C ABI, for the test/bench harness.

Buffers may be numpy arrays (host memory) or torch tensors (host or HBM); the
library itself decides per pointer whether to stage it.  Nothing here computes
a distance: every function forwards to libpgv_hip.so.
"""
import ctypes as C
import weakref

import numpy as np

from . import _lib
from ._lib import (PGV_ERR_ARG, PGV_ERR_STATE, PGV_F16, PGV_F32, PGV_L1, PGV_L2SQ, PGV_NEG_IP, PGV_OPS_COSINE,  # noqa: F401
                   PGV_OPS_IP, PGV_OPS_L2, PgvError, PgvRng, PgvStats, check, lib)

_NP_OF = {PGV_F32: np.float32, PGV_F16: np.float16}


def _is_torch(x):
    return type(x).__module__.startswith("torch")


def ptr(x):
    """raw address of a numpy array / torch tensor (None -> NULL)"""
    if x is None:
        return None
    if _is_torch(x):
        assert x.is_contiguous(), "tensor must be contiguous"
        return C.c_void_p(x.data_ptr())
    assert isinstance(x, np.ndarray) and x.flags["C_CONTIGUOUS"], "need a C-contiguous array"
    return C.c_void_p(x.ctypes.data)


def _on_device(x):
    return _is_torch(x) and x.is_cuda


def _empty_like_kind(ref, shape, np_dtype):
    """output buffer living where `ref` lives"""
    if _on_device(ref):
        import torch
        return torch.empty(shape, dtype=getattr(torch, np.dtype(np_dtype).name), device=ref.device)
    return np.empty(shape, dtype=np_dtype)


def as_dtype(x, dtype):
    """host arrays: make sure element type and layout match what the ABI reads"""
    if _is_torch(x):
        return x.contiguous()
    return np.ascontiguousarray(x, dtype=_NP_OF[dtype])


def live_words(mask):
    """[n] booleans -> the (n + 31) / 32 uint32 words pgv_hnsw_set_live takes: element e is bit e & 31 of word e >> 5"""
    mask = np.ascontiguousarray(np.asarray(mask).ravel() != 0)
    padded = np.zeros(((mask.size + 31) // 32) * 32, dtype=bool)
    padded[:mask.size] = mask
    return np.ascontiguousarray(np.packbits(padded, bitorder="little").view("<u4").astype(np.uint32))


def make_rng(seed=0, next_double=None, next_u32=None, state=None):
    """pgv_rng: the library's own generator (seed) or caller callbacks (C function pointers)"""
    r = PgvRng()
    r.next_double = C.cast(next_double, C.c_void_p) if next_double is not None else None
    r.next_u32 = C.cast(next_u32, C.c_void_p) if next_u32 is not None else None
    r.state = state
    r.seed = seed
    return r


class Context:
    def __init__(self, device=0, stream=None):
        """stream: None -> a private stream; an int hipStream_t handle -> enqueue on that stream
        (0, the handle of the default stream, is passed as PGV_DEFAULT_STREAM)"""
        h = C.c_void_p()
        if stream is None:
            arg = None
        elif stream == 0:
            arg = C.c_void_p(-1)  # PGV_DEFAULT_STREAM
        else:
            arg = C.c_void_p(stream)
        check(lib.pgv_ctx_create(device, arg, C.byref(h)))
        self.h = h
        self.device = device
        self._children = []  # weakrefs: index/hnsw handles must be freed before their context

    def _adopt(self, child):
        self._children.append(weakref.ref(child))

    def close(self):
        if self.h:
            for ref in self._children:
                child = ref()
                if child is not None:
                    child.close()
            self._children = []
            lib.pgv_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def sync(self):
        check(lib.pgv_ctx_sync(self.h))

    def stream(self):
        return lib.pgv_ctx_stream(self.h)

    def timer_start(self):
        check(lib.pgv_timer_start(self.h))

    def timer_stop(self):
        ms = C.c_float()
        check(lib.pgv_timer_stop(self.h, C.byref(ms)))
        return ms.value

    def set_profiling(self, on):
        check(lib.pgv_ctx_set_profiling(self.h, 1 if on else 0))

    def set_exact_scan(self, on):
        """Keep batched L2 scans on the exact vector-ALU kernels (no matrix-core pre-filter)."""
        check(lib.pgv_ctx_set_exact_scan(self.h, 1 if on else 0))

    def set_bound(self, worst_case):
        """pgv_ctx_set_bound: the rounding bound the MFMA L2 paths prove completeness with (statistical / worst case)"""
        check(lib.pgv_ctx_set_bound(self.h, _lib.PGV_BOUND_WORST_CASE if worst_case else _lib.PGV_BOUND_STATISTICAL))

    def reset_stats(self):
        check(lib.pgv_ctx_reset_stats(self.h))

    def stats(self):
        s = PgvStats()
        check(lib.pgv_ctx_get_stats(self.h, C.byref(s)))
        return {"scan_ms": s.scan_ms, "scan_launches": s.scan_launches,
                "scan_pairs": s.scan_pairs, "scan_rows": s.scan_rows,
                "aux_ms": s.aux_ms, "aux_launches": s.aux_launches, "aux_pairs": s.aux_pairs,
                "assign_redo_rows": s.assign_redo_rows, "assign_rows": s.assign_rows,
                "assign_recheck_rows": s.assign_recheck_rows, "scan_unique_rows": s.scan_unique_rows, "scan_redo_queries": s.scan_redo_queries,
                "scan_widened_queries": s.scan_widened_queries, "scan_pruned_probes": s.scan_pruned_probes,
                "scan_shadow_queries": s.scan_shadow_queries}


class IvfIndex:
    """device mirror of one IVFFlat index (pgv_index_upload)"""

    def __init__(self, ctx, metric, dtype, dim, centers, list_offsets, vectors, tids=None):
        self.ctx, self.metric, self.dtype, self.dim = ctx, metric, dtype, dim
        centers = as_dtype(centers, dtype)
        vectors = as_dtype(vectors, dtype)
        if not _is_torch(list_offsets):
            list_offsets = np.ascontiguousarray(list_offsets, dtype=np.int64)
        if tids is not None and not _is_torch(tids):
            tids = np.ascontiguousarray(tids, dtype=np.uint64)
        self.nlists = int(list_offsets.shape[0]) - 1
        h = C.c_void_p()
        check(lib.pgv_index_upload(ctx.h, metric, dtype, dim, self.nlists, ptr(centers),
                                   ptr(list_offsets), ptr(vectors), ptr(tids), C.byref(h)))
        self.h = h
        ctx._adopt(self)

    def set_overlap(self, lanes):
        """pgv_index_set_overlap: consecutive search_batch calls run on `lanes` internal streams in turn (one batch's
        ranking / planning / top-k under the other's scan); device outputs are complete after ctx.sync().  1 = off."""
        check(lib.pgv_index_set_overlap(self.h, int(lanes)))

    def share(self, ctx):
        """a second handle for another context (its own stream and scratch) on the same device: pgv_index_share.
        The device arrays go with the last handle that is closed."""
        v = IvfIndex.__new__(IvfIndex)
        v.ctx, v.metric, v.dtype, v.dim, v.nlists = ctx, self.metric, self.dtype, self.dim, self.nlists
        h = C.c_void_p()
        check(lib.pgv_index_share(self.h, ctx.h, C.byref(h)))
        v.h = h
        ctx._adopt(v)
        return v

    def export(self):
        """pgv_index_export: the 256-byte handle another PROCESS imports (pgv_index_import) to scan this mirror"""
        buf = C.create_string_buffer(256)
        check(lib.pgv_index_export(self.h, buf))
        return bytes(buf.raw)

    @classmethod
    def from_handle(cls, ctx, handle, metric=None, dtype=None, dim=None):
        """pgv_index_import: map a mirror another process exported (no copy)"""
        v = cls.__new__(cls)
        h = C.c_void_p()
        buf = C.create_string_buffer(bytes(handle), 256)
        check(lib.pgv_index_import(ctx.h, buf, C.byref(h)))
        v.ctx, v.metric, v.dtype, v.dim, v.h = ctx, metric, dtype, dim, h
        v.nlists = lib.pgv_index_lists(h)
        ctx._adopt(v)
        return v

    def close(self):
        if self.h:
            lib.pgv_index_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def rows(self):
        return lib.pgv_index_rows(self.h)

    def tids(self, slots):
        """pgv_index_tids: heap TIDs of row slots, for a caller without a TID table (a backend that imported)"""
        slots = np.ascontiguousarray(slots, dtype=np.int64)
        out = np.empty(slots.shape, dtype=np.uint64)
        check(lib.pgv_index_tids(self.h, ptr(slots), int(slots.size), ptr(out)))
        return out

    def rank_lists(self, queries, maxprobes, want_dist=True):
        queries = as_dtype(queries, self.dtype)
        nq = int(queries.shape[0])
        lists = _empty_like_kind(queries, (nq, maxprobes), np.int32)
        dist = _empty_like_kind(queries, (nq, maxprobes), np.float32) if want_dist else None
        check(lib.pgv_rank_lists(self.h, ptr(queries), nq, maxprobes, ptr(lists), ptr(dist)))
        return lists, dist

    def scan_lists(self, query, lists):
        if query is not None:
            query = as_dtype(query, self.dtype)
        lists = np.ascontiguousarray(lists, dtype=np.int32)
        count = C.c_int64()
        # first call sizes the output (capacity 0 only reports the count)
        rc = lib.pgv_scan_lists(self.h, ptr(query), ptr(lists), len(lists), None, None, 0, C.byref(count))
        if rc != _lib.PGV_OK and count.value == 0:
            check(rc)
        m = count.value
        dist = np.empty(m, dtype=np.float32)
        slot = np.empty(m, dtype=np.int64)
        if m:
            check(lib.pgv_scan_lists(self.h, ptr(query), ptr(lists), len(lists), ptr(dist), ptr(slot),
                                     m, C.byref(count)))
        return dist, slot

    def search_batch(self, queries, probes, k, want_tid=False, out=None):
        queries = as_dtype(queries, self.dtype)
        nq = int(queries.shape[0])
        if out is None:
            dist = _empty_like_kind(queries, (nq, k), np.float32)
            slot = _empty_like_kind(queries, (nq, k), np.int64)
            tid = _empty_like_kind(queries, (nq, k), np.uint64 if not _on_device(queries) else np.int64) \
                if want_tid else None
        else:
            dist, slot, tid = out
        check(lib.pgv_search_batch(self.h, ptr(queries), nq, probes, k, ptr(dist), ptr(slot), ptr(tid)))
        return dist, slot, tid


def _scan_batch(self, queries, probe_lists, k, want_tid=False, out=None):
    """GetScanItems + sorted head for probe lists chosen elsewhere (pgv_scan_batch)"""
    queries = as_dtype(queries, self.dtype)
    nq = int(queries.shape[0])
    if not _is_torch(probe_lists):
        probe_lists = np.ascontiguousarray(probe_lists, dtype=np.int32)
    probes = int(probe_lists.shape[1])
    if out is None:
        dist = _empty_like_kind(queries, (nq, k), np.float32)
        slot = _empty_like_kind(queries, (nq, k), np.int64)
        tid = _empty_like_kind(queries, (nq, k), np.uint64 if not _on_device(queries) else np.int64) \
            if want_tid else None
    else:
        dist, slot, tid = out
    check(lib.pgv_scan_batch(self.h, ptr(queries), nq, ptr(probe_lists), probes, k, ptr(dist), ptr(slot),
                             ptr(tid)))
    return dist, slot, tid


IvfIndex.scan_batch = _scan_batch


class Query:
    """one backend's index scan, device-resident between calls (pgv_query_*): rank() = GetScanLists,
    scan() = GetScanItems + the sorted head, more() = deeper into the same batch's sorted stream"""

    def __init__(self, index):
        self.index = index
        h = C.c_void_p()
        check(lib.pgv_query_begin(index.h, C.byref(h)))
        self.h = h
        index.ctx._adopt(self)

    def close(self):
        if self.h:
            lib.pgv_query_end(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def rank(self, query, max_probes):
        if query is not None:
            query = as_dtype(query, self.index.dtype)
        self._q = query
        check(lib.pgv_query_rank(self.h, ptr(query), int(max_probes)))

    def lists(self, n):
        out = np.empty(n, dtype=np.int32)
        check(lib.pgv_query_lists(self.h, ptr(out), n))
        return out

    def scan(self, first, nprobes, head, want_tid=True):
        dist = np.empty(head, dtype=np.float32)
        slot = np.empty(head, dtype=np.int64)
        tid = np.empty(head, dtype=np.uint64) if want_tid else None
        count, total = C.c_int(), C.c_int64()
        check(lib.pgv_query_scan(self.h, int(first), int(nprobes), int(head), ptr(dist), ptr(slot), ptr(tid),
                                 C.byref(count), C.byref(total)))
        n = count.value
        return dist[:n], slot[:n], (tid[:n] if want_tid else None), total.value

    def more(self, skip, count, want_tid=True):
        dist = np.empty(count, dtype=np.float32)
        slot = np.empty(count, dtype=np.int64)
        tid = np.empty(count, dtype=np.uint64) if want_tid else None
        got = C.c_int()
        check(lib.pgv_query_more(self.h, int(skip), int(count), ptr(dist), ptr(slot), ptr(tid), C.byref(got)))
        n = got.value
        return dist[:n], slot[:n], (tid[:n] if want_tid else None)


class Comm:
    """one process per GPU: the library's communicator (pgv_comm_*).  backend "rccl": RCCL over xGMI, the
    group id travels through torch.distributed once; backend "host": the two collectives are callbacks into
    torch.distributed -- through host memory under gloo (functional runs only), through device staging tensors under
    torch's nccl backend (RCCL driven by torch: what bench.py falls back to when pgv_comm_create fails)."""

    def __init__(self, ctx, backend="rccl"):
        import torch
        import torch.distributed as dist
        self.ctx = ctx
        self.world = dist.get_world_size() if dist.is_initialized() else 1
        self.rank = dist.get_rank() if dist.is_initialized() else 0
        h = C.c_void_p()
        if backend == "rccl":
            ident = torch.zeros(128, dtype=torch.uint8)
            if self.world > 1:
                if self.rank == 0:
                    buf = (C.c_uint8 * 128)()
                    check(lib.pgv_comm_unique_id(buf))
                    ident = torch.tensor(list(buf), dtype=torch.uint8)
                on_dev = dist.get_backend() == "nccl"
                t = ident.cuda() if on_dev else ident
                dist.broadcast(t, 0)
                ident = t.cpu()
            if self.world == 1:  # a group of one: still through RCCL, which exercises the plumbing on one GPU
                buf = (C.c_uint8 * 128)()
                check(lib.pgv_comm_unique_id(buf))
                ident = torch.tensor(list(buf), dtype=torch.uint8)
            raw = (C.c_uint8 * 128)(*ident.tolist())
            check(lib.pgv_comm_create(ctx.h, self.world, self.rank, raw, C.byref(h)))
        else:
            hip = C.CDLL("libamdhip64.so")
            hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
            hip.hipStreamSynchronize.argtypes = [C.c_void_p]
            world = self.world
            # the staging tensors live where torch.distributed's backend wants them: host memory for gloo, this
            # device for nccl (= RCCL driven by torch: the fallback when pgv_comm_create itself cannot be had)
            on_dev = dist.is_initialized() and dist.get_backend() == "nccl"
            where = torch.device("cuda", ctx.device) if on_dev else torch.device("cpu")
            to_stage, from_stage = (3, 3) if on_dev else (2, 1)   # hipMemcpyKind: D2D / D2H, H2D

            def all_reduce(_state, buf, count, stream):
                try:
                    hip.hipStreamSynchronize(stream)
                    stage = torch.empty(count, dtype=torch.float32, device=where)
                    hip.hipMemcpy(stage.data_ptr(), buf, count * 4, to_stage)
                    dist.all_reduce(stage)
                    if on_dev:
                        torch.cuda.synchronize(where)
                    hip.hipMemcpy(buf, stage.data_ptr(), count * 4, from_stage)
                    return 0
                except Exception:
                    return 1

            def all_gather(_state, send, recv, nbytes, stream):
                try:
                    hip.hipStreamSynchronize(stream)
                    mine = torch.empty(nbytes, dtype=torch.uint8, device=where)
                    hip.hipMemcpy(mine.data_ptr(), send, nbytes, to_stage)
                    full = torch.empty(nbytes * world, dtype=torch.uint8, device=where)
                    dist.all_gather_into_tensor(full, mine) if on_dev else dist.all_gather(list(full.split(nbytes)), mine)
                    if on_dev:
                        torch.cuda.synchronize(where)
                    hip.hipMemcpy(recv, full.data_ptr(), nbytes * world, from_stage)
                    return 0
                except Exception:
                    return 1
            self._cbs = (_lib.ALL_REDUCE_F32(all_reduce), _lib.ALL_GATHER(all_gather))
            coll = _lib.PgvCollectives(self._cbs[0], self._cbs[1], None)
            self._coll = coll
            check(lib.pgv_comm_create_custom(ctx.h, self.world, self.rank, C.byref(coll), C.byref(h)))
        self.h = h
        ctx._adopt(self)

    def close(self):
        if self.h:
            lib.pgv_comm_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def kmeans(self, ops, dtype, dim, samples_local, k, rng=None, max_iterations=500, want_closest=True):
        samples_local = as_dtype(samples_local, dtype)
        n = int(samples_local.shape[0])
        centers = _empty_like_kind(samples_local, (k, dim), _NP_OF[dtype])
        closest = _empty_like_kind(samples_local, (n,), np.int32) if want_closest and n else None
        iters = C.c_int()
        check(lib.pgv_kmeans_sharded(self.h, ops, dtype, dim, ptr(samples_local) if n else None, n, k, max_iterations,
                                     C.byref(rng) if rng is not None else None, ptr(centers), ptr(closest),
                                     C.byref(iters)))
        return centers, closest, iters.value

    def search_batch(self, index, queries, probes, k, out=None):
        queries = as_dtype(queries, index.dtype)
        nq = int(queries.shape[0])
        if out is None:
            dist_ = _empty_like_kind(queries, (nq, k), np.float32)
            tid = _empty_like_kind(queries, (nq, k), np.uint64 if not _on_device(queries) else np.int64)
        else:
            dist_, tid = out
        check(lib.pgv_search_batch_sharded(self.h, index.h, ptr(queries), nq, probes, k, ptr(dist_), ptr(tid)))
        return dist_, tid


def assign(ctx, metric, dtype, dim, centers, rows, want_dist=True):
    centers = as_dtype(centers, dtype)
    rows = as_dtype(rows, dtype)
    n = int(rows.shape[0])
    out = _empty_like_kind(rows, (n,), np.int32)
    dist = _empty_like_kind(rows, (n,), np.float32) if want_dist else None
    check(lib.pgv_assign(ctx.h, metric, dtype, dim, ptr(centers), int(centers.shape[0]), ptr(rows), n,
                         ptr(out), ptr(dist)))
    return out, dist


def distance_batch(ctx, metric, dtype, dim, query, rows):
    query = as_dtype(query, dtype)
    rows = as_dtype(rows, dtype)
    n = int(rows.shape[0])
    out = _empty_like_kind(rows, (n,), np.float32)
    check(lib.pgv_distance_batch(ctx.h, metric, dtype, dim, ptr(query), ptr(rows), n, ptr(out)))
    return out


def exact_topk(ctx, metric, dtype, dim, queries, rows, k, out=None):
    """pgv_exact_topk: the index-less `ORDER BY <op> LIMIT k` for a batch of queries -> (dist [nq x k], idx [nq x k])"""
    queries = as_dtype(queries, dtype)
    rows = as_dtype(rows, dtype)
    nq, n = int(queries.shape[0]), int(rows.shape[0])
    dist, idx = out if out is not None else (_empty_like_kind(queries, (nq, k), np.float32),
                                            _empty_like_kind(queries, (nq, k), np.int64))
    check(lib.pgv_exact_topk(ctx.h, metric, dtype, dim, ptr(queries), nq, ptr(rows) if n else None, n, int(k),
                             ptr(dist), ptr(idx)))
    return dist, idx


def kmeans(ctx, ops, dtype, dim, samples, k, rng=None, max_iterations=500, want_closest=True):
    samples = as_dtype(samples, dtype)
    n = int(samples.shape[0])
    centers = _empty_like_kind(samples, (k, dim), _NP_OF[dtype])
    closest = _empty_like_kind(samples, (n,), np.int32) if want_closest and n else None
    iters = C.c_int()
    check(lib.pgv_kmeans(ctx.h, ops, dtype, dim, ptr(samples) if n else None, n, k, max_iterations,
                         C.byref(rng) if rng is not None else None, ptr(centers), ptr(closest),
                         C.byref(iters)))
    return centers, closest, iters.value


def kmeanspp_init(ctx, ops, dtype, dim, samples, k, rng=None):
    samples = as_dtype(samples, dtype)
    centers = _empty_like_kind(samples, (k, dim), _NP_OF[dtype])
    check(lib.pgv_kmeanspp_init(ctx.h, ops, dtype, dim, ptr(samples), int(samples.shape[0]), k,
                                C.byref(rng) if rng is not None else None, ptr(centers)))
    return centers


def lloyd_partial(ctx, ops, dtype, dim, samples, centers, closest):
    """closest is updated in place; returns (sums [k x dim] fp32, counts [k], changes)"""
    samples = as_dtype(samples, dtype)
    centers = as_dtype(centers, dtype)
    k = int(centers.shape[0])
    n = int(samples.shape[0])
    sums = _empty_like_kind(samples, (k, dim), np.float32)
    counts = _empty_like_kind(samples, (k,), np.int32)
    changes = _empty_like_kind(samples, (1,), np.int64)
    check(lib.pgv_lloyd_partial(ctx.h, ops, dtype, dim, ptr(samples), n, ptr(centers), k, ptr(closest),
                                ptr(sums), ptr(counts), ptr(changes)))
    return sums, counts, changes


def lloyd_finish(ctx, ops, dtype, dim, sums, counts, rng=None, like=None):
    k = int(counts.shape[0])
    centers = _empty_like_kind(like if like is not None else sums, (k, dim), _NP_OF[dtype])
    check(lib.pgv_lloyd_finish(ctx.h, ops, dtype, dim, k, ptr(sums), ptr(counts),
                               C.byref(rng) if rng is not None else None, ptr(centers)))
    return centers


def cosine_distance_batch(ctx, dtype, dim, query, rows):
    """cosine_distance of one query against n rows, float8 like the operator (pgv_cosine_distance_batch)"""
    query, rows = as_dtype(query, dtype), as_dtype(rows, dtype)
    n = int(rows.shape[0])
    out = _empty_like_kind(rows, (n,), np.float64)
    check(lib.pgv_cosine_distance_batch(ctx.h, dtype, dim, ptr(query), ptr(rows), n, ptr(out)))
    return out


PGV_BIT_HAMMING, PGV_BIT_JACCARD = 0, 1


def bit_distance_batch(ctx, metric, nbits, query, rows):
    """hamming / jaccard distance of one packed bit string against n packed rows [n x (nbits + 7) // 8] uint8"""
    if not _is_torch(rows):
        rows = np.ascontiguousarray(rows, dtype=np.uint8)
        query = np.ascontiguousarray(query, dtype=np.uint8)
    n = int(rows.shape[0])
    out = _empty_like_kind(rows, (n,), np.float64)
    check(lib.pgv_bit_distance_batch(ctx.h, metric, nbits, ptr(query) if nbits else None, ptr(rows), n, ptr(out)))
    return out


def _as_bytes(x):
    return x.contiguous() if _is_torch(x) else np.ascontiguousarray(x, dtype=np.uint8)


def bit_topk(ctx, nbits, queries, rows, k, out=None):
    """pgv_bit_topk: `ORDER BY b <~> $1 LIMIT k` for a batch of packed bit strings: queries [nq x (nbits + 7) // 8] uint8
    against rows [n x (nbits + 7) // 8] uint8 -> (dist [nq x k] float32, idx [nq x k] int64), ties to the lower row"""
    queries, rows = _as_bytes(queries), _as_bytes(rows)
    nq, n = int(queries.shape[0]), int(rows.shape[0])
    dist, idx = out if out is not None else (_empty_like_kind(queries, (nq, k), np.float32),
                                            _empty_like_kind(queries, (nq, k), np.int64))
    check(lib.pgv_bit_topk(ctx.h, int(nbits), ptr(queries) if nbits and nq else None, nq, ptr(rows) if nbits and n else None, n,
                           int(k), ptr(dist), ptr(idx)))
    return dist, idx


_CSR_DTYPES = (np.int64, np.int32, np.float32)


def _csr(triple):
    """a CSR triple (ptr [n + 1], idx [ptr[n]], val [ptr[n]]) as the ABI reads it: int64, int32, float32.  Host arrays are
    converted; tensors must already have those element types"""
    out = []
    for x, dt in zip(triple, _CSR_DTYPES):
        if _is_torch(x):
            assert str(x.dtype) == "torch." + np.dtype(dt).name, "CSR tensors: int64 ptr, int32 idx, float32 val"
            out.append(x.contiguous())
        else:
            out.append(np.ascontiguousarray(x, dtype=dt))
    return out


def sparse_distance_batch(ctx, metric, dim, query, rows):
    """pgv_sparse_distance_batch: one sparse query (idx [nnz], val [nnz]) against CSR rows (ptr, idx, val) -> [n] float32
    kernel values (L2 squared / negative inner product / L1), living where the rows' values live"""
    _, q_idx, q_val = _csr((np.zeros(1, dtype=np.int64),) + tuple(query))
    r_ptr, r_idx, r_val = _csr(rows)
    n = int(r_ptr.shape[0]) - 1
    out = _empty_like_kind(r_val, (n,), np.float32)
    check(lib.pgv_sparse_distance_batch(ctx.h, metric, int(dim), int(q_idx.shape[0]), ptr(q_idx), ptr(q_val), ptr(r_ptr),
                                        ptr(r_idx), ptr(r_val), n, ptr(out)))
    return out


def sparse_cosine_distance_batch(ctx, dim, query, rows):
    """pgv_sparse_cosine_distance_batch: cosine_distance of one sparse query against CSR rows, float8 like the operator"""
    _, q_idx, q_val = _csr((np.zeros(1, dtype=np.int64),) + tuple(query))
    r_ptr, r_idx, r_val = _csr(rows)
    n = int(r_ptr.shape[0]) - 1
    out = _empty_like_kind(r_val, (n,), np.float64)
    check(lib.pgv_sparse_cosine_distance_batch(ctx.h, int(dim), int(q_idx.shape[0]), ptr(q_idx), ptr(q_val), ptr(r_ptr),
                                               ptr(r_idx), ptr(r_val), n, ptr(out)))
    return out


def sparse_topk(ctx, metric, dim, queries, rows, k, out=None):
    """pgv_sparse_topk: the index-less `ORDER BY <op> LIMIT k` over sparsevec for a batch: CSR queries and CSR rows
    (ptr, idx, val) -> (dist [nq x k] float32, idx [nq x k] int64), ties to the lower row, living where the queries'
    values live"""
    q_ptr, q_idx, q_val = _csr(queries)
    r_ptr, r_idx, r_val = _csr(rows)
    nq, n = int(q_ptr.shape[0]) - 1, int(r_ptr.shape[0]) - 1
    dist, idx = out if out is not None else (_empty_like_kind(q_val, (nq, k), np.float32),
                                            _empty_like_kind(q_val, (nq, k), np.int64))
    check(lib.pgv_sparse_topk(ctx.h, metric, int(dim), ptr(q_ptr), ptr(q_idx), ptr(q_val), nq, ptr(r_ptr), ptr(r_idx),
                              ptr(r_val), n, int(k), ptr(dist), ptr(idx)))
    return dist, idx


def binary_quantize(ctx, dtype, dim, rows):
    """pgv_binary_quantize: rows [n x dim] -> packed bits [n x (dim + 7) // 8] uint8, bit i = rows[:, i] > 0, first element
    in the top bit of byte 0 (np.packbits' order)"""
    rows = as_dtype(rows, dtype)
    n = int(rows.shape[0])
    out = _empty_like_kind(rows, (n, (dim + 7) // 8), np.uint8)
    check(lib.pgv_binary_quantize(ctx.h, dtype, dim, ptr(rows) if n else None, n, ptr(out)))
    return out


def rerank(ctx, metric, dtype, dim, queries, rows, cand, k):
    """pgv_rerank: exact kernel values of each query against its own candidate rows cand [nq x kc] int64 (-1 = none)
    -> (dist [nq x k], idx [nq x k]), ties to the lower candidate position"""
    queries, rows = as_dtype(queries, dtype), as_dtype(rows, dtype)
    cand = cand.contiguous() if _is_torch(cand) else np.ascontiguousarray(cand, dtype=np.int64)
    nq, n, kc = int(queries.shape[0]), int(rows.shape[0]), int(cand.shape[1])
    dist = _empty_like_kind(queries, (nq, k), np.float32)
    idx = _empty_like_kind(queries, (nq, k), np.int64)
    check(lib.pgv_rerank(ctx.h, metric, dtype, dim, ptr(queries), nq, ptr(rows) if n else None, n, ptr(cand), kc, int(k),
                         ptr(dist), ptr(idx)))
    return dist, idx


def binary_search(ctx, metric, dtype, dim, queries, rows, bits, kc, k, want_candidates=False):
    """the two-stage query of binary quantization: quantise the queries, the kc nearest rows of `bits` (the rows'
    binary_quantize image) by Hamming distance, then the k nearest of those by the exact metric over `rows`
    -> (dist [nq x k], idx [nq x k]) and, on request, stage one's (hamming [nq x kc], cand [nq x kc])"""
    qbits = binary_quantize(ctx, dtype, dim, queries)
    hamming, cand = bit_topk(ctx, dim, qbits, bits, kc)
    dist, idx = rerank(ctx, metric, dtype, dim, queries, rows, cand, k)
    return (dist, idx, hamming, cand) if want_candidates else (dist, idx)


class BitIvfIndex(IvfIndex):
    """device mirror of `USING ivfflat (col bit_hamming_ops)` (pgv_index_upload_bits): centers [nlists x (nbits + 7) // 8]
    and rows [n x (nbits + 7) // 8] uint8, first bit in the top bit of byte 0 (np.packbits' order), pad bits zero.
    rank_lists, scan_lists, search_batch and scan_batch take packed queries and return Hamming distances as float32
    (exact); share, tids, rows and close are IvfIndex's.  set_overlap, export and Query are refused by the library."""

    def __init__(self, ctx, nbits, centers, list_offsets, rows, tids=None):
        self.ctx, self.metric, self.dtype, self.dim, self.nbits = ctx, None, None, int(nbits), int(nbits)
        centers, rows = _as_bytes(centers), _as_bytes(rows)
        if not _is_torch(list_offsets):
            list_offsets = np.ascontiguousarray(list_offsets, dtype=np.int64)
        if tids is not None and not _is_torch(tids):
            tids = np.ascontiguousarray(tids, dtype=np.uint64)
        self.nlists = int(list_offsets.shape[0]) - 1
        h = C.c_void_p()
        check(lib.pgv_index_upload_bits(ctx.h, int(nbits), self.nlists, ptr(centers), ptr(list_offsets),
                                        ptr(rows) if int(rows.shape[0]) else None, ptr(tids), C.byref(h)))
        self.h = h
        ctx._adopt(self)

    def share(self, ctx):
        v = BitIvfIndex.__new__(BitIvfIndex)
        v.ctx, v.metric, v.dtype, v.dim, v.nbits, v.nlists = ctx, None, None, self.dim, self.nbits, self.nlists
        h = C.c_void_p()
        check(lib.pgv_index_share(self.h, ctx.h, C.byref(h)))
        v.h = h
        ctx._adopt(v)
        return v

    def rank_lists(self, queries, maxprobes, want_dist=True):
        queries = _as_bytes(queries)
        nq = int(queries.shape[0])
        lists = _empty_like_kind(queries, (nq, maxprobes), np.int32)
        dist = _empty_like_kind(queries, (nq, maxprobes), np.float32) if want_dist else None
        check(lib.pgv_rank_lists(self.h, ptr(queries), nq, maxprobes, ptr(lists), ptr(dist)))
        return lists, dist

    def scan_lists(self, query, lists, capacity=None):
        """-> (dist [m], slot [m]) in stream order; capacity: the output size offered (default: what the lists hold)"""
        if query is not None:
            query = _as_bytes(query)
        lists = np.ascontiguousarray(lists, dtype=np.int32)
        count = C.c_int64()
        if capacity is None:
            rc = lib.pgv_scan_lists(self.h, ptr(query), ptr(lists), len(lists), None, None, 0, C.byref(count))
            if rc != _lib.PGV_OK and count.value == 0:
                check(rc)
            capacity = count.value
        dist = np.empty(capacity, dtype=np.float32)
        slot = np.empty(capacity, dtype=np.int64)
        check(lib.pgv_scan_lists(self.h, ptr(query), ptr(lists), len(lists), ptr(dist), ptr(slot), int(capacity),
                                 C.byref(count)))
        return dist[:count.value], slot[:count.value]

    def _outputs(self, queries, nq, k, want_tid, out):
        if out is not None:
            return out
        return (_empty_like_kind(queries, (nq, k), np.float32), _empty_like_kind(queries, (nq, k), np.int64),
                _empty_like_kind(queries, (nq, k), np.uint64 if not _on_device(queries) else np.int64) if want_tid else None)

    def search_batch(self, queries, probes, k, want_tid=False, out=None):
        queries = _as_bytes(queries)
        nq = int(queries.shape[0])
        dist, slot, tid = self._outputs(queries, nq, k, want_tid, out)
        check(lib.pgv_search_batch(self.h, ptr(queries), nq, int(probes), int(k), ptr(dist), ptr(slot), ptr(tid)))
        return dist, slot, tid

    def scan_batch(self, queries, probe_lists, k, want_tid=False, out=None):
        queries = _as_bytes(queries)
        nq = int(queries.shape[0])
        if not _is_torch(probe_lists):
            probe_lists = np.ascontiguousarray(probe_lists, dtype=np.int32)
        dist, slot, tid = self._outputs(queries, nq, k, want_tid, out)
        check(lib.pgv_scan_batch(self.h, ptr(queries), nq, ptr(probe_lists), int(probe_lists.shape[1]), int(k), ptr(dist),
                                 ptr(slot), ptr(tid)))
        return dist, slot, tid


def bit_assign(ctx, nbits, centers, rows, want_dist=True):
    """pgv_bit_assign: the first strictly-nearest center of every packed row under Hamming distance
    -> (list [n] int32, dist [n] float32 or None)"""
    centers, rows = _as_bytes(centers), _as_bytes(rows)
    n = int(rows.shape[0])
    out = _empty_like_kind(rows, (n,), np.int32)
    dist = _empty_like_kind(rows, (n,), np.float32) if want_dist else None
    check(lib.pgv_bit_assign(ctx.h, int(nbits), ptr(centers), int(centers.shape[0]), ptr(rows) if n else None, n, ptr(out),
                             ptr(dist)))
    return out, dist


def bit_kmeans(ctx, nbits, samples, k, rng=None, max_iterations=500, want_closest=True):
    """pgv_bit_kmeans: IvfflatKmeans for bit strings -> (centers [k x bytes] uint8, closest [n] int32 or None, iterations)"""
    samples = _as_bytes(samples)
    n = int(samples.shape[0])
    centers = _empty_like_kind(samples, (k, (int(nbits) + 7) // 8), np.uint8)
    closest = _empty_like_kind(samples, (n,), np.int32) if want_closest and n else None
    iters = C.c_int()
    check(lib.pgv_bit_kmeans(ctx.h, int(nbits), ptr(samples) if n else None, n, int(k), int(max_iterations),
                             C.byref(rng) if rng is not None else None, ptr(centers), ptr(closest), C.byref(iters)))
    return centers, closest, iters.value


def bit_lloyd_step(ctx, nbits, samples, centers, closest, rng=None):
    """pgv_bit_lloyd_step: one iteration of pgv_bit_kmeans; closest (int32, -1 = not assigned yet) is updated in place
    -> (new centers [k x bytes] uint8, counts [k] int32, changes)"""
    samples, centers = _as_bytes(samples), _as_bytes(centers)
    n, k = int(samples.shape[0]), int(centers.shape[0])
    new = _empty_like_kind(centers, (k, (int(nbits) + 7) // 8), np.uint8)
    counts = np.empty(k, dtype=np.int32)
    changes = np.empty(1, dtype=np.int64)
    check(lib.pgv_bit_lloyd_step(ctx.h, int(nbits), ptr(samples) if n else None, n, ptr(centers), k, ptr(closest),
                                 C.byref(rng) if rng is not None else None, ptr(new), ptr(counts), ptr(changes)))
    return new, counts, int(changes[0])


def build_bit_ivf(ctx, nbits, rows, lists, rng=None, samples=None):
    """`CREATE INDEX ... USING ivfflat (col bit_hamming_ops) WITH (lists = ...)` from the library's pieces: k-means over
    `samples` (default: all rows), pgv_bit_assign, a stable sort by list (heap order inside a list) and the upload, with
    the row index as the TID -> (BitIvfIndex, centers [lists x bytes], list_offsets [lists + 1])"""
    rows = np.ascontiguousarray(rows, dtype=np.uint8)
    centers, _, _ = bit_kmeans(ctx, nbits, rows if samples is None else samples, lists, rng=rng, want_closest=False)
    assigned, _ = bit_assign(ctx, nbits, centers, rows, want_dist=False)
    order = np.argsort(assigned, kind="stable")
    offsets = np.zeros(lists + 1, dtype=np.int64)
    offsets[1:] = np.cumsum(np.bincount(assigned, minlength=lists))
    index = BitIvfIndex(ctx, nbits, centers, offsets, rows[order], tids=order.astype(np.uint64))
    return index, centers, offsets


def binary_search_ivf(ctx, metric, dtype, dim, queries, rows, bit_ivf, probes, kc, k, want_candidates=False):
    """the two-stage query of binary quantization over an IVFFlat index of the rows' binary_quantize image (a BitIvfIndex
    whose TIDs are the row indexes, as build_bit_ivf uploads them): quantise the queries, the kc nearest tuples of the
    `probes` nearest lists by Hamming distance, then the k nearest of those by the exact metric over `rows`
    -> (dist [nq x k], idx [nq x k]) and, on request, stage one's (hamming [nq x kc], cand [nq x kc])"""
    qbits = binary_quantize(ctx, dtype, dim, queries)
    hamming, slot, tid = bit_ivf.search_batch(qbits, probes, kc, want_tid=True)
    if _is_torch(tid):
        cand = tid  # (int64 on the device: the "none" TID ~0 reads as -1)
    else:
        cand = np.where(slot >= 0, tid.astype(np.int64), -1)
    dist, idx = rerank(ctx, metric, dtype, dim, queries, rows, cand, k)
    return (dist, idx, hamming, cand) if want_candidates else (dist, idx)


class IvfBuilder:
    """pgv_builder_*: heap rows assigned and kept on the device, finish() = the tuplesort by list as a device gather
    whose result is the mirror itself"""

    def __init__(self, ctx, metric, dtype, dim, centers, expected_rows=0, nlists=None):
        """centers None (and nlists given): they come with set_centers(); add() only uploads until then"""
        self.ctx, self.metric, self.dtype, self.dim = ctx, metric, dtype, dim
        if centers is not None:
            centers = as_dtype(centers, dtype)
            nlists = int(centers.shape[0])
        self.nlists = int(nlists)
        h = C.c_void_p()
        check(lib.pgv_builder_begin(ctx.h, metric, dtype, dim, self.nlists, ptr(centers), int(expected_rows), C.byref(h)))
        self.h = h

    def set_centers(self, centers):
        centers = as_dtype(centers, self.dtype)
        if int(centers.shape[0]) != self.nlists:
            raise ValueError("set_centers: %d centers for %d lists" % (centers.shape[0], self.nlists))
        check(lib.pgv_builder_set_centers(self.h, ptr(centers)))

    def add(self, rows, tids=None):
        rows = as_dtype(rows, self.dtype)
        if tids is not None and not _is_torch(tids):
            tids = np.ascontiguousarray(tids, dtype=np.uint64)
        check(lib.pgv_builder_add(self.h, ptr(rows), ptr(tids), int(rows.shape[0])))

    @property
    def rows(self):
        return lib.pgv_builder_rows(self.h)

    def finish(self, want_lists=False):
        """-> (IvfIndex, list_offsets [lists + 1], lists [rows, heap order] or None)"""
        n = self.rows
        off = np.empty(self.nlists + 1, dtype=np.int64)
        lists = np.empty(n, dtype=np.int32) if want_lists else None
        h = C.c_void_p()
        check(lib.pgv_builder_finish(self.h, C.byref(h), ptr(off), ptr(lists)))
        ix = IvfIndex.__new__(IvfIndex)
        ix.ctx, ix.metric, ix.dtype, ix.dim, ix.h = self.ctx, self.metric, self.dtype, self.dim, h
        ix.nlists = self.nlists
        self.ctx._adopt(ix)
        return ix, off, lists

    def close(self):
        if self.h:
            lib.pgv_builder_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_SINK = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p)


def drain_index(index, chunk_rows=0):
    """pgv_index_drain -> (vectors [n x dim], tids [n]) in list-major order (host copies; a test helper)"""
    n = index.rows
    npdt = _NP_OF[index.dtype]
    vec = np.empty((n, index.dim), dtype=npdt)
    tids = np.zeros(n, dtype=np.uint64)
    row_bytes = index.dim * vec.itemsize
    seen = []

    def sink(_arg, first, count, vptr, tptr):
        C.memmove(vec.ctypes.data + first * row_bytes, vptr, count * row_bytes)
        if tptr:
            C.memmove(tids.ctypes.data + first * 8, tptr, count * 8)
        seen.append((first, count))
        return 0
    cb = _SINK(sink)
    check(lib.pgv_index_drain(index.h, int(chunk_rows), cb, None))
    return vec, tids, seen


class Hnsw:
    """device mirror of an HNSW index's element vectors (pgv_hnsw_upload)"""

    def __init__(self, ctx, metric, dtype, dim, elements, payload=None):
        """payload: [n x w] uint32 per-element words kept next to the vectors (pgv_hnsw_upload_payload)"""
        self.ctx, self.metric, self.dtype, self.dim = ctx, metric, dtype, dim
        elements = as_dtype(elements, dtype)
        h = C.c_void_p()
        if payload is None:
            check(lib.pgv_hnsw_upload(ctx.h, metric, dtype, dim, ptr(elements), int(elements.shape[0]),
                                      C.byref(h)))
            self.payload_words = 0
        else:
            payload = np.ascontiguousarray(payload, dtype=np.uint32)
            self.payload_words = int(payload.shape[1])
            check(lib.pgv_hnsw_upload_payload(ctx.h, metric, dtype, dim, ptr(elements), int(elements.shape[0]),
                                              ptr(payload), 4 * self.payload_words, C.byref(h)))
        self.h = h
        ctx._adopt(self)

    def get_payload(self, elements, words=None):
        """pgv_hnsw_get_payload: the payload rows of result elements -> [n x w] uint32 (zeros for slots < 0)"""
        elements = np.ascontiguousarray(elements, dtype=np.int64).ravel()
        w = words or self.payload_words
        out = np.empty((elements.size, w), dtype=np.uint32)
        check(lib.pgv_hnsw_get_payload(self.h, ptr(elements), int(elements.size), ptr(out)))
        return out

    def close(self):
        if self.h:
            lib.pgv_hnsw_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def export(self):
        """pgv_hnsw_export: the handle another PROCESS imports (pgv_hnsw_import) to search this mirror"""
        buf = C.create_string_buffer(256)
        check(lib.pgv_hnsw_export(self.h, buf))
        return bytes(buf.raw)

    @classmethod
    def from_handle(cls, ctx, handle, dtype):
        """pgv_hnsw_import: map the elements and the graph another process exported (no copy, read-only)"""
        v = cls.__new__(cls)
        h = C.c_void_p()
        buf = C.create_string_buffer(bytes(handle), 256)
        check(lib.pgv_hnsw_import(ctx.h, buf, C.byref(h)))
        v.ctx, v.metric, v.dtype, v.dim, v.h = ctx, None, dtype, None, h
        v.payload_words = 0
        ctx._adopt(v)
        return v

    def share(self, ctx):
        """pgv_hnsw_share: a view of this mirror for another context of the same process (own stream and scratch; the
        vectors and the graph stay this mirror's).  Close the view before the mirror."""
        v = Hnsw.__new__(Hnsw)
        h = C.c_void_p()
        check(lib.pgv_hnsw_share(self.h, ctx.h, C.byref(h)))
        v.ctx, v.metric, v.dtype, v.dim, v.h = ctx, self.metric, self.dtype, self.dim, h
        v.payload_words = self.payload_words
        v._owner = self   # keeps the owner alive
        ctx._adopt(v)
        return v

    def update_graph(self, entry, elements, tuple_offsets, tuples):
        """pgv_hnsw_update_graph: new entry point and the rewritten neighbor tuples of `elements` (tuple i =
        tuples[tuple_offsets[i] : tuple_offsets[i + 1]]); through a view the patch lands in the owner's graph"""
        elements = np.ascontiguousarray(elements, dtype=np.int32)
        tuple_offsets = np.ascontiguousarray(tuple_offsets, dtype=np.int64)
        tuples = np.ascontiguousarray(tuples, dtype=np.int32)
        check(lib.pgv_hnsw_update_graph(self.h, int(entry), ptr(elements), int(elements.size), ptr(tuple_offsets),
                                        ptr(tuples)))
        self._graph = None

    def set_graph(self, m, entry, levels, nbr_start, nbr):
        """the graph a scan walks (pgv_hnsw_set_graph): per element slot its level and neighbor tuple"""
        levels = np.ascontiguousarray(levels, dtype=np.int32) if not _is_torch(levels) else levels
        nbr_start = np.ascontiguousarray(nbr_start, dtype=np.int64) if not _is_torch(nbr_start) else nbr_start
        nbr = np.ascontiguousarray(nbr, dtype=np.int32) if not _is_torch(nbr) else nbr
        check(lib.pgv_hnsw_set_graph(self.h, int(m), int(entry), ptr(levels), ptr(nbr_start), ptr(nbr)))
        # (host arrays are remembered for repair(); update_graph forgets them)
        self._graph = None if _is_torch(levels) or _is_torch(nbr_start) or _is_torch(nbr) else (int(entry), levels, nbr_start, nbr)

    def set_live(self, mask):
        """pgv_hnsw_set_live: mask [n] of booleans, True = the element still has heap TIDs (None: every element is live
        again).  Only the repair search reads it; searches and scans walk through dead elements as before."""
        if mask is None:
            check(lib.pgv_hnsw_set_live(self.h, None, 0))
            return
        words = live_words(mask)
        check(lib.pgv_hnsw_set_live(self.h, ptr(words), int(words.size)))

    def live_count(self):
        """pgv_hnsw_live_count: the elements not marked dead"""
        return int(lib.pgv_hnsw_live_count(self.h))

    def repair(self, mask, m, ef_construction, max_batch=1024, graph=None, dead_cap=0):
        """pgv_host_hnsw_repair: hnswvacuum's RepairGraph after the elements with mask[e] == False lost their heap TIDs.
        graph = (entry, levels, nbr_start, nbr), host arrays; None: the arrays of the last set_graph / repair of this
        object.  Returns a dict: the new nbr and entry (levels and nbr_start do not change) and the counters; the mirror
        holds the repaired graph and the bitmap afterwards.  max_batch = 1 is the reference's serial loop."""
        from . import _host
        if graph is None:
            graph = getattr(self, "_graph", None)
            if graph is None:
                raise PgvError(PGV_ERR_STATE, "Hnsw.repair: no graph given and none set through this object (set_graph)")
        entry, levels, nbr_start, nbr = graph
        out = _host.hnsw_repair(self, entry, levels, nbr_start, nbr, live_words(mask), m, ef_construction, max_batch, dead_cap)
        self._graph = (out["entry"], levels, nbr_start, out["nbr"])
        return out

    def repair_dead_cap_max(self, ef_construction):
        """the largest dead_cap of repair_neighbors whose W fits a workgroup's LDS (-1: none)"""
        return int(lib.pgv_hnsw_repair_dead_cap_max(self.h, int(ef_construction)))

    def repair_neighbors(self, elements, m, ef_construction, layer_cap, dead_cap):
        """pgv_hnsw_repair_neighbors: HnswFindElementNeighbors(existing = true) for a batch of linked elements ->
        (ids, dist, closer [nq x layer_cap x 2m], count [nq x layer_cap], status [nq] (1: W overflowed dead_cap, counts 0),
        pair distances computed).  m is the graph's (set_graph)."""
        elements = np.ascontiguousarray(elements, dtype=np.int32).ravel()
        nq, stride = int(elements.size), 2 * int(m)
        ids = np.full((nq, layer_cap, stride), -1, dtype=np.int32)
        dist = np.zeros((nq, layer_cap, stride), dtype=np.float32)
        closer = np.zeros((nq, layer_cap, stride), dtype=np.uint8)
        count = np.zeros((nq, layer_cap), dtype=np.int32)
        status = np.zeros((nq,), dtype=np.int32)
        pairs = C.c_int64(0)
        check(lib.pgv_hnsw_repair_neighbors(self.h, ptr(elements), nq, int(ef_construction), int(layer_cap), int(dead_cap),
                                            ptr(ids), ptr(dist), ptr(closer), ptr(count), ptr(status), C.byref(pairs)))
        return ids, dist, closer, count, status, int(pairs.value)

    def search(self, queries, ef_search, k, want_scored=True):
        """hnswgettuple's first batch on the device (pgv_hnsw_search) ->
        (element slots [nq x k] nearest first / -1, distances [nq x k] / +inf, scored [nq] or None)"""
        queries = as_dtype(queries, self.dtype)
        nq = int(queries.shape[0])
        elem = _empty_like_kind(queries, (nq, k), np.int64)
        dist = _empty_like_kind(queries, (nq, k), np.float32)
        scored = _empty_like_kind(queries, (nq,), np.int64) if want_scored else None
        check(lib.pgv_hnsw_search(self.h, ptr(queries), nq, int(ef_search), int(k), ptr(elem), ptr(dist),
                                  ptr(scored)))
        return elem, dist, scored

    def scan(self, queries, ef_search, discard_cap=0):
        """pgv_hnsw_scan_begin: a resumable scan of these queries (hnsw.iterative_scan) -> HnswScan"""
        return HnswScan(self, as_dtype(queries, self.dtype), ef_search, discard_cap)

    def score(self, queries, slot, query_of=None):
        queries = as_dtype(queries, self.dtype)
        slot = np.ascontiguousarray(slot, dtype=np.int32) if not _is_torch(slot) else slot
        if query_of is not None and not _is_torch(query_of):
            query_of = np.ascontiguousarray(query_of, dtype=np.int32)
        n = int(slot.shape[0])
        out = _empty_like_kind(slot, (n,), np.float32)
        check(lib.pgv_hnsw_score(self.h, ptr(queries), int(queries.shape[0]), ptr(slot), ptr(query_of),
                                 n, ptr(out)))
        return out


class BitHnsw(Hnsw):
    """device mirror of an HNSW index over packed bit strings, `USING hnsw (... bit_hamming_ops)` (pgv_hnsw_upload_bits):
    elements [n x (nbits + 7) // 8] uint8, first bit in the top bit of byte 0 (np.packbits' order), pad bits zero.
    set_graph, update_graph, get_payload, export and close are Hnsw's; search and score take packed queries and return
    Hamming distances as float32 (exact).  buildable=True uploads through pgv_hnsw_upload_bits_buildable: the same mirror,
    which the build-side entries serve as well (_host.hnsw_build builds its graph)."""

    def __init__(self, ctx, nbits, elements, payload=None, metric=PGV_BIT_HAMMING, buildable=False):
        self.ctx, self.metric, self.dtype, self.dim, self.nbits = ctx, metric, None, int(nbits), int(nbits)
        self.buildable = bool(buildable)
        elements = _as_bytes(elements)
        n = int(elements.shape[0])
        h = C.c_void_p()
        self.payload_words = 0
        if payload is not None:
            payload = np.ascontiguousarray(payload, dtype=np.uint32)
            self.payload_words = int(payload.shape[1])
        upload = lib.pgv_hnsw_upload_bits_buildable if buildable else lib.pgv_hnsw_upload_bits
        check(upload(ctx.h, int(metric), int(nbits), ptr(elements) if n else None, n, ptr(payload), 4 * self.payload_words,
                     C.byref(h)))
        self.h = h
        ctx._adopt(self)

    @classmethod
    def from_handle(cls, ctx, handle, nbits=None):
        """pgv_hnsw_import of a bit mirror's export: the handle carries the element type and nbits"""
        v = super().from_handle(ctx, handle, None)
        v.nbits = nbits
        v.buildable = False  # (the handle does not carry it: importers do not build)
        return v

    def share(self, ctx):
        v = type(self).__new__(type(self))
        h = C.c_void_p()
        check(lib.pgv_hnsw_share(self.h, ctx.h, C.byref(h)))
        v.ctx, v.metric, v.dtype, v.dim, v.nbits, v.h = ctx, self.metric, None, self.dim, self.nbits, h
        v.buildable = getattr(self, "buildable", False)
        v.payload_words = self.payload_words
        v._owner = self   # keeps the owner alive
        ctx._adopt(v)
        return v

    def search(self, queries, ef_search, k, want_scored=True):
        """pgv_hnsw_search on a bit mirror: queries [nq x (nbits + 7) // 8] uint8 ->
        (element slots [nq x k] nearest first / -1, Hamming distances [nq x k] float32 / +inf, scored [nq] or None)"""
        queries = _as_bytes(queries)
        nq = int(queries.shape[0])
        elem = _empty_like_kind(queries, (nq, k), np.int64)
        dist = _empty_like_kind(queries, (nq, k), np.float32)
        scored = _empty_like_kind(queries, (nq,), np.int64) if want_scored else None
        check(lib.pgv_hnsw_search(self.h, ptr(queries), nq, int(ef_search), int(k), ptr(elem), ptr(dist), ptr(scored)))
        return elem, dist, scored

    def scan(self, queries, ef_search, discard_cap=0):
        """pgv_hnsw_scan_begin on a bit mirror: packed queries as search takes them -> HnswScan"""
        return HnswScan(self, _as_bytes(queries), ef_search, discard_cap)

    def score(self, queries, slot, query_of=None):
        """pgv_hnsw_score on a bit mirror: Hamming distance of element slot[i] to packed query query_of[i]"""
        queries = _as_bytes(queries)
        slot = np.ascontiguousarray(slot, dtype=np.int32) if not _is_torch(slot) else slot
        if query_of is not None and not _is_torch(query_of):
            query_of = np.ascontiguousarray(query_of, dtype=np.int32)
        n = int(slot.shape[0])
        out = _empty_like_kind(slot, (n,), np.float32)
        check(lib.pgv_hnsw_score(self.h, ptr(queries), int(queries.shape[0]), ptr(slot), ptr(query_of), n, ptr(out)))
        return out

    def score_pairs(self, a, b):
        """pgv_hnsw_score_pairs: Hamming distance between element slots a[i] and b[i]"""
        a, b = np.ascontiguousarray(a, dtype=np.int32), np.ascontiguousarray(b, dtype=np.int32)
        out = np.empty((a.size,), dtype=np.float32)
        check(lib.pgv_hnsw_score_pairs(self.h, ptr(a), ptr(b), int(a.size), ptr(out)))
        return out


class JaccardHnsw(BitHnsw):
    """device mirror of an HNSW index over packed bit strings under `USING hnsw (... bit_jaccard_ops)`
    (pgv_hnsw_upload_jaccard): elements as BitHnsw takes them.  The walk ranks by an integer key of the Jaccard ratio that
    orders and ties exactly as the reference's float8 does; search, scan, score and score_pairs return Jaccard distances,
    each the float32 of the reference's float8 for the pair (1.0 when the strings share no bit).  set_graph, update_graph,
    get_payload, export and close are Hnsw's.  The graph comes from the reference's build, or, with buildable=True
    (pgv_hnsw_upload_bits_buildable under PGV_BIT_JACCARD), from _host.hnsw_build on this mirror."""

    def __init__(self, ctx, nbits, elements, payload=None, buildable=False):
        if buildable:
            BitHnsw.__init__(self, ctx, nbits, elements, payload=payload, metric=PGV_BIT_JACCARD, buildable=True)
            return
        self.ctx, self.metric, self.dtype, self.dim, self.nbits = ctx, PGV_BIT_JACCARD, None, int(nbits), int(nbits)
        self.buildable = False
        elements = _as_bytes(elements)
        n = int(elements.shape[0])
        h = C.c_void_p()
        self.payload_words = 0
        if payload is not None:
            payload = np.ascontiguousarray(payload, dtype=np.uint32)
            self.payload_words = int(payload.shape[1])
        check(lib.pgv_hnsw_upload_jaccard(ctx.h, int(nbits), ptr(elements) if n else None, n, ptr(payload),
                                          4 * self.payload_words, C.byref(h)))
        self.h = h
        ctx._adopt(self)

    @classmethod
    def from_handle(cls, ctx, handle, nbits=None):
        """pgv_hnsw_import of a Jaccard mirror's export: the handle carries nbits and the bit metric, so the importer
        walks with Jaccard keys whichever bit class opens it"""
        v = super().from_handle(ctx, handle, nbits)
        v.metric = PGV_BIT_JACCARD
        return v

    def share(self, ctx):
        """pgv_hnsw_share: a view of this Jaccard mirror for another context of the same process"""
        return super().share(ctx)


class SparseHnsw(Hnsw):
    """device mirror of an HNSW index over sparsevec elements, `USING hnsw (... sparsevec_l2_ops / _ip_ops / _cosine_ops /
    _l1_ops)` (pgv_hnsw_upload_sparse): rows_csr = (ptr [n + 1], idx, val) as sparse_topk takes them, at most 1000 stored
    elements per element; metric PGV_L2SQ / PGV_NEG_IP / PGV_L1 (cosine: PGV_NEG_IP over normalised vectors).
    set_graph, update_graph, get_payload and close are Hnsw's; search, score and score_pairs take CSR queries / element
    slots and return sparse_distance_batch's values; scan_sparse begins a resumable scan (hnsw.iterative_scan) with CSR
    queries.  No export: the mirror is not shared across processes.
    buildable=True uploads through pgv_hnsw_upload_sparse_buildable: the same mirror, which the build-side entries serve as
    well (_host.hnsw_build(mirror, None, m, ef_construction, rows_csr=...) builds its graph); views inherit it."""

    sparse = True

    def __init__(self, ctx, metric, dim, rows_csr, payload=None, buildable=False):
        self.ctx, self.metric, self.dtype, self.dim = ctx, metric, None, int(dim)
        self.buildable = bool(buildable)
        r_ptr, r_idx, r_val = _csr(rows_csr)
        n = int(r_ptr.shape[0]) - 1
        h = C.c_void_p()
        self.payload_words = 0
        if payload is not None:
            payload = np.ascontiguousarray(payload, dtype=np.uint32)
            self.payload_words = int(payload.shape[1])
        upload = lib.pgv_hnsw_upload_sparse_buildable if buildable else lib.pgv_hnsw_upload_sparse
        check(upload(ctx.h, int(metric), int(dim), ptr(r_ptr), ptr(r_idx), ptr(r_val), n, ptr(payload), 4 * self.payload_words,
                     C.byref(h)))
        self.h = h
        ctx._adopt(self)

    def share(self, ctx):
        v = SparseHnsw.__new__(SparseHnsw)
        h = C.c_void_p()
        check(lib.pgv_hnsw_share(self.h, ctx.h, C.byref(h)))
        v.ctx, v.metric, v.dtype, v.dim, v.h = ctx, self.metric, None, self.dim, h
        v.buildable = getattr(self, "buildable", False)
        v.payload_words = self.payload_words
        v._owner = self   # keeps the owner alive
        ctx._adopt(v)
        return v

    def search(self, queries_csr, ef_search, k, want_scored=True):
        """pgv_hnsw_search_sparse: CSR queries (a query may store up to 16 000 elements) ->
        (element slots [nq x k] nearest first / -1, distances [nq x k] float32 / +inf, scored [nq] or None)"""
        q_ptr, q_idx, q_val = _csr(queries_csr)
        nq = int(q_ptr.shape[0]) - 1
        elem = _empty_like_kind(q_val, (nq, k), np.int64)
        dist = _empty_like_kind(q_val, (nq, k), np.float32)
        scored = _empty_like_kind(q_val, (nq,), np.int64) if want_scored else None
        check(lib.pgv_hnsw_search_sparse(self.h, ptr(q_ptr), ptr(q_idx), ptr(q_val), nq, int(ef_search), int(k), ptr(elem),
                                         ptr(dist), ptr(scored)))
        return elem, dist, scored

    def scan(self, queries_csr, ef_search, discard_cap=0):
        raise PgvError(PGV_ERR_ARG, "scan takes dense query rows (pgv_hnsw_scan_begin): a sparse mirror is scanned "
                                    "iteratively with scan_sparse")

    def scan_sparse(self, queries_csr, ef_search, discard_cap=0):
        """pgv_hnsw_scan_begin_sparse: a resumable scan of these CSR queries (hnsw.iterative_scan) -> SparseHnswScan, with
        HnswScan's interface; the scan keeps its own copy of the queries"""
        return SparseHnswScan(self, queries_csr, ef_search, discard_cap)

    def score(self, queries_csr, slot, query_of=None):
        """pgv_hnsw_score_sparse: the distance of element slot[i] to query query_of[i] (None: query 0) of the CSR queries"""
        q_ptr, q_idx, q_val = _csr(queries_csr)
        slot = np.ascontiguousarray(slot, dtype=np.int32) if not _is_torch(slot) else slot
        if query_of is not None and not _is_torch(query_of):
            query_of = np.ascontiguousarray(query_of, dtype=np.int32)
        n = int(slot.shape[0])
        out = _empty_like_kind(slot, (n,), np.float32)
        check(lib.pgv_hnsw_score_sparse(self.h, ptr(q_ptr), ptr(q_idx), ptr(q_val), int(q_ptr.shape[0]) - 1, ptr(slot),
                                        ptr(query_of), n, ptr(out)))
        return out

    def score_pairs(self, a, b):
        """pgv_hnsw_score_pairs: the distance of element a[i] to element b[i], b[i] taken as the query"""
        a, b = np.ascontiguousarray(a, dtype=np.int32), np.ascontiguousarray(b, dtype=np.int32)
        out = np.empty((a.size,), dtype=np.float32)
        check(lib.pgv_hnsw_score_pairs(self.h, ptr(a), ptr(b), int(a.size), ptr(out)))
        return out


def _host_array(x):
    return x.cpu().numpy() if _is_torch(x) else np.asarray(x)


def pack_keep(keep):
    """a filter over element slots as pgv_hnsw_scan_filtered reads it: boolean [n] (one filter for every query) or
    [nq, n] (one per query) -> uint32 words [(n + 31) / 32] or [nq, (n + 31) / 32], element e at bit e & 31 of word
    e >> 5.  A boolean tensor is packed where it lives (as int32 words: torch's 32-bit type), a few filters at a time: the
    temporaries stay below about 128 MB whatever nq is"""
    if _is_torch(keep):
        import torch
        n = int(keep.shape[-1])
        words = (n + 31) // 32
        rows = keep.reshape(-1, n)
        out = torch.empty((rows.shape[0], words), dtype=torch.int32, device=keep.device)
        weights = torch.tensor([1, 2, 4, 8, 16, 32, 64, 128], dtype=torch.uint8, device=keep.device)
        step = max(1, (32 << 20) // (words * 32))
        for lo in range(0, rows.shape[0], step):
            part = rows[lo:lo + step]
            bits = torch.zeros((part.shape[0], words * 32), dtype=torch.uint8, device=keep.device)
            bits[:, :n] = part != 0
            # eight bits a byte (their weights sum to 255 at the most), four bytes a word, the lowest first
            out[lo:lo + step] = (bits.view(-1, words * 4, 8) * weights).sum(-1, dtype=torch.uint8).view(torch.int32)
        return out.reshape(tuple(keep.shape[:-1]) + (words,))
    keep = np.asarray(keep) != 0
    n = keep.shape[-1]
    words = (n + 31) // 32
    bits = np.zeros(keep.shape[:-1] + (words * 32,), dtype=np.uint8)
    bits[..., :n] = keep
    return np.ascontiguousarray(np.packbits(bits, axis=-1, bitorder="little")).view("<u4").reshape(keep.shape[:-1] + (words,))


def _is_keep_words(keep):
    """a filter that is packed already: 32-bit integers, an array or a tensor"""
    if _is_torch(keep):
        return str(keep.dtype) in ("torch.int32", "torch.uint32")
    return isinstance(keep, np.ndarray) and keep.dtype in (np.uint32, np.int32)


class HnswScan:
    """a resumable scan over a batch of queries (pgv_hnsw_scan_*): hnswgettuple's batches, one launch each.  Close it
    before the mirror it scans."""

    def __init__(self, mirror, queries, ef_search, discard_cap=0):
        self.mirror, self.nq, self.ef = mirror, int(queries.shape[0]), int(ef_search)
        self._like = queries
        s = C.c_void_p()
        check(lib.pgv_hnsw_scan_begin(mirror.h, ptr(queries) if self.nq else None, self.nq, self.ef, int(discard_cap),
                                      C.byref(s)))
        self.s = s

    def _want(self, want):
        if want is None:
            return None
        want = np.ascontiguousarray(np.asarray(want) != 0, dtype=np.uint8)
        assert want.shape == (self.nq,)
        return want

    def next(self, want=None):
        """pgv_hnsw_scan_next: the next batch of the wanted queries (None: all) -> (element slots [nq x ef] nearest
        first / -1, distances [nq x ef] / +inf, count [nq], scored [nq]: so->tuples so far, left [nq]: pool entries)"""
        want = self._want(want)
        elem = _empty_like_kind(self._like, (self.nq, self.ef), np.int64)
        dist = _empty_like_kind(self._like, (self.nq, self.ef), np.float32)
        count = _empty_like_kind(self._like, (self.nq,), np.int32)
        scored = _empty_like_kind(self._like, (self.nq,), np.int64)
        left = _empty_like_kind(self._like, (self.nq,), np.int64)
        check(lib.pgv_hnsw_scan_next(self.s, ptr(want), ptr(elem), ptr(dist), ptr(count), ptr(scored), ptr(left)))
        return elem, dist, count, scored, left

    def drain(self, count, want=None):
        """pgv_hnsw_scan_drain: the `count` nearest pool entries of the wanted queries, removed from their pools ->
        (element slots [nq x count] / -1, distances / +inf, count [nq])"""
        want = self._want(want)
        count = int(count)
        shape = (self.nq, max(count, 1))
        elem = _empty_like_kind(self._like, shape, np.int64)
        dist = _empty_like_kind(self._like, shape, np.float32)
        got = _empty_like_kind(self._like, (self.nq,), np.int32)
        check(lib.pgv_hnsw_scan_drain(self.s, ptr(want), count, ptr(elem), ptr(dist), ptr(got)))
        return elem, dist, got

    def filtered(self, k, keep=None, max_scan_tuples=20000, strict=False, want=None):
        """pgv_hnsw_scan_filtered: hnswgettuple's loop under a filter for the wanted queries (None: all), one launch --
        batches through `keep` until a query has k rows, is exhausted or, past max_scan_tuples, has drained its pool.
        keep: None (every element), a boolean array or tensor [n] or [nq, n] over element slots (packed with pack_keep),
        or an array or tensor of 32-bit integers [words] or [nq, words] that is such a bitmap already (words >= (n + 31) /
        32), passed through as it is.  n is the mirror's element count: any other length is refused here.
        -> (element slots [nq x k] in emission order / -1, distances [nq x k] / +inf, count [nq], scored [nq]: so->tuples
        at the end, batches [nq]: walks plus drains taken, left [nq]: pool entries)"""
        want = self._want(want)
        k = int(k)
        stride = 0
        if keep is not None:
            n = int(lib.pgv_hnsw_elements(self.mirror.h))
            if _is_keep_words(keep):
                if int(keep.shape[-1]) < (n + 31) // 32:
                    raise PgvError(PGV_ERR_ARG, "keep: %d words, the mirror's %d elements take %d" % (keep.shape[-1], n, (n + 31) // 32))
                keep = keep.contiguous() if _is_torch(keep) else np.ascontiguousarray(keep)
            else:
                if int(keep.shape[-1]) != n:
                    raise PgvError(PGV_ERR_ARG, "keep: a filter over %d elements, the mirror has %d" % (keep.shape[-1], n))
                keep = pack_keep(keep)
            if keep.ndim not in (1, 2) or (keep.ndim == 2 and keep.shape[0] != self.nq):
                raise PgvError(PGV_ERR_ARG, "keep: one filter [n] or one per query [%d, n]" % self.nq)
            stride = int(keep.shape[1]) if keep.ndim == 2 else 0
        shape = (self.nq, max(k, 1))
        elem = _empty_like_kind(self._like, shape, np.int64)
        dist = _empty_like_kind(self._like, shape, np.float32)
        count = _empty_like_kind(self._like, (self.nq,), np.int32)
        scored = _empty_like_kind(self._like, (self.nq,), np.int64)
        batches = _empty_like_kind(self._like, (self.nq,), np.int32)
        left = _empty_like_kind(self._like, (self.nq,), np.int64)
        check(lib.pgv_hnsw_scan_filtered(self.s, ptr(want), ptr(keep), stride, k, int(max_scan_tuples), int(bool(strict)),
                                         ptr(elem), ptr(dist), ptr(count), ptr(scored), ptr(batches), ptr(left)))
        return elem, dist, count, scored, batches, left

    def close(self):
        if self.s:
            lib.pgv_hnsw_scan_end(self.s)
            self.s = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class SparseHnswScan(HnswScan):
    """HnswScan over a sparse mirror (pgv_hnsw_scan_begin_sparse): the queries in CSR, as SparseHnsw.search takes them"""

    def __init__(self, mirror, queries_csr, ef_search, discard_cap=0):
        q_ptr, q_idx, q_val = _csr(queries_csr)
        self.mirror, self.nq, self.ef = mirror, int(q_ptr.shape[0]) - 1, int(ef_search)
        self._like = q_val
        self.s = None
        s = C.c_void_p()
        check(lib.pgv_hnsw_scan_begin_sparse(mirror.h, ptr(q_ptr), ptr(q_idx), ptr(q_val), self.nq, self.ef, int(discard_cap),
                                             C.byref(s)))
        self.s = s


def hnsw_iterative_search(h, queries, k, keep, ef_search, max_scan_tuples=20000, strict=False, discard_cap=0):
    """hnswgettuple's loop (src/hnswscan.c:242-327) under hnsw.iterative_scan over a batch of queries: batches nearest
    first, `keep` (a boolean array over element slots, the executor's filter) applied to each, with `strict` an element
    nearer than the last one emitted dropped (:313-319), a query stopped at k kept elements; once its so->tuples
    reaches max_scan_tuples a query takes the remaining discarded candidates instead of walking on (:259-266).  Only the
    queries that still want more advance.  A SparseHnsw takes its queries in CSR.  -> (ids: per query the kept element
    slots in emission order, dist: their distances, scored [nq]: so->tuples at the end)"""
    keep = np.asarray(keep, dtype=bool)
    begin = h.scan_sparse if getattr(h, "sparse", False) else h.scan
    with begin(queries, ef_search, discard_cap) as s:
        nq = s.nq
        ids, dist = [[] for _ in range(nq)], [[] for _ in range(nq)]
        prev = np.full(nq, -np.inf)
        scored = np.zeros(nq, dtype=np.int64)
        walking, draining = np.ones(nq, dtype=bool), np.zeros(nq, dtype=bool)

        def emit(q, elems, dists):
            ok = keep[elems]
            if strict:  # an element nearer than the last one emitted is dropped: `prev` is the largest distance seen
                seen = np.maximum.accumulate(np.concatenate([prev[q:q + 1], dists]))
                ok &= dists >= seen[:-1]
                prev[q] = seen[-1]
            room = k - len(ids[q])
            ids[q] += elems[ok][:room].tolist()
            dist[q] += dists[ok][:room].tolist()

        while walking.any() or draining.any():
            if walking.any():
                e, d, c, sc, _left = (_host_array(x) for x in s.next(walking))
                for q in np.flatnonzero(walking):
                    scored[q] = sc[q]
                    emit(q, e[q, :c[q]], d[q, :c[q]])
                    if c[q] == 0 or len(ids[q]) >= k:
                        walking[q] = False
                    elif sc[q] >= max_scan_tuples:
                        walking[q], draining[q] = False, True
            if draining.any():
                e, d, c = (_host_array(x) for x in s.drain(ef_search, draining))
                for q in np.flatnonzero(draining):
                    emit(q, e[q, :c[q]], d[q, :c[q]])
                    if c[q] == 0 or len(ids[q]) >= k:
                        draining[q] = False
    return ids, dist, scored


def hnsw_filtered_search(h, queries, k, keep, ef_search, max_scan_tuples=20000, strict=False, discard_cap=0):
    """hnsw_iterative_search with the loop on the device: one scan, one pgv_hnsw_scan_filtered launch, one copy back.
    keep: as HnswScan.filtered takes it.  A SparseHnsw takes its queries in CSR.  -> (ids: per query the kept element
    slots in emission order, dist: their distances, scored [nq]: so->tuples at the end)"""
    begin = h.scan_sparse if getattr(h, "sparse", False) else h.scan
    with begin(queries, ef_search, discard_cap) as s:
        elem, dist, count, scored, _batches, _left = (_host_array(x) for x in s.filtered(k, keep, max_scan_tuples, strict))
    ids = [elem[q, :count[q]].tolist() for q in range(s.nq)]
    return ids, [dist[q, :count[q]].tolist() for q in range(s.nq)], scored.astype(np.int64)


def binary_search_hnsw(ctx, metric, dtype, dim, queries, rows, bit_hnsw, ef_search, kc, k, want_candidates=False):
    """the INDEXED two-stage query of binary quantization (the reference README's `USING hnsw (... bit_hamming_ops)`
    form): quantise the queries, the kc <= ef_search nearest elements of `bit_hnsw` (a BitHnsw over the rows'
    binary_quantize image, element slot i = row i) by walking its graph, then the k nearest of those by the exact metric
    over `rows` -> (dist [nq x k], idx [nq x k]) and, on request, stage one's (hamming [nq x kc], cand [nq x kc], scored)"""
    qbits = binary_quantize(ctx, dtype, dim, queries)
    cand, hamming, scored = bit_hnsw.search(qbits, ef_search, kc)
    dist, idx = rerank(ctx, metric, dtype, dim, queries, rows, cand, k)
    return (dist, idx, hamming, cand, scored) if want_candidates else (dist, idx)
