"""Thin torch-tensor wrappers over the libmirec.so C-ABI (include/mirec.h).

Every device function here launches a hand-written gfx950 kernel on the current
HIP stream. Inputs must already be device tensors of the stated dtype; nothing is
copied to the host and nothing falls back to PyTorch or the CPU — a tensor on
the wrong device or a missing library raises. The host_* functions are the
library's CPU data-pipeline primitives (numpy arrays in and out).
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from recbole_amd._native import NativeError, check, lib, ptr, stream_handle

# Per-launch HIP events of named kernels, collected while a dict is installed here
# ({name: [(start, end), ...]}; tools/bench_models.py): the measuring tool times a
# model step's dominant kernel on the stream it runs on. None: no events.
KERNEL_EVENTS = None


class timed_launch(object):
    """`with timed_launch(name): <one native launch>` — records a start / end event pair
    on the current stream when KERNEL_EVENTS holds `name` (nothing otherwise)."""

    def __init__(self, name):
        self.name = name
        self.ev = None

    def __enter__(self):
        if KERNEL_EVENTS is not None and self.name in KERNEL_EVENTS:
            self.ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            self.ev[0].record()
        return self

    def __exit__(self, *exc):
        if self.ev is not None:
            self.ev[1].record()
            KERNEL_EVENTS[self.name].append(self.ev)
        return False


def _dev(t: torch.Tensor, dtype, name: str) -> torch.Tensor:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if not t.is_cuda:
        raise NativeError(f"{name} must live on the GPU (got {t.device}); no CPU fallback exists")
    if t.dtype != dtype:
        raise TypeError(f"{name} must be {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    return t


# ---------------------------------------------------------------- K4 sampler
def sample_walk(random_list: torch.Tensor, pr_dev: torch.Tensor, keys: torch.Tensor, num: int,
                used_ptr: torch.Tensor | None, used_cols: torch.Tensor | None, n_key_space: int,
                reject: bool, batch_keys: int | None = None, n_batches: int = 1,
                out: torch.Tensor | None = None, status: torch.Tensor | None = None,
                ws: torch.Tensor | None = None, out_stride: int = 0,
                used_bits: torch.Tensor | None = None, n_bits: int = 0) -> torch.Tensor:
    """Bit-exact cyclic-walk negative sampling (sampler.py:82-154). Membership
    comes from `used_bits` (see used_bitmap) when given, else the CSR."""
    _dev(random_list, torch.int32, "random_list")
    _dev(pr_dev, torch.int64, "pr_dev")
    _dev(keys, torch.int64, "keys")
    n_keys = keys.numel()
    if batch_keys is None:
        batch_keys = max(n_keys, 1)
    if out is None:
        out = torch.empty(n_keys * num, dtype=torch.int64, device=keys.device)
    if status is None:
        status = torch.zeros(1, dtype=torch.int32, device=keys.device)
    if reject and used_bits is None:
        _dev(used_ptr, torch.int64, "used_ptr")
        _dev(used_cols, torch.int32, "used_cols")
    if reject and used_bits is not None:
        _dev(used_bits, torch.int32, "used_bits")
    wsz = lib().mirec_sample_walk_workspace_size(batch_keys, num)
    if ws is None or ws.numel() < wsz:
        ws = torch.empty(wsz, dtype=torch.uint8, device=keys.device)
    bits = reject and used_bits is not None
    rc = lib().mirec_sample_walk(ptr(random_list), random_list.numel(), ptr(pr_dev), ptr(keys),
                                 n_keys, batch_keys, n_batches, num,
                                 ptr(used_ptr) if reject and not bits else None,
                                 ptr(used_cols) if reject and not bits else None,
                                 ptr(used_bits) if bits else None, n_bits if bits else 0,
                                 n_key_space,
                                 1 if reject else 0, ptr(out), out_stride, ptr(status), ptr(ws),
                                 ws.numel(),
                                 stream_handle())
    check(rc, "mirec_sample_walk")
    return out


def sample_walk_spec(random_list: torch.Tensor, pr_dev: torch.Tensor, users: torch.Tensor,
                     batch_keys: int, n_batches: int, num: int, used_ptr, used_cols,
                     n_key_space: int, reject: bool, r_mean: float, r_sd: float,
                     out: torch.Tensor | None = None, out_stride: int = 0, status=None,
                     used_bits=None, n_bits: int = 0, items=None, user_keys=None,
                     item_keys=None, key_stride: int = 0) -> torch.Tensor:
    """K4s (mirec_sample_walk_spec): the walk of n_batches batches of batch_keys keys
    (users[b*batch_keys:]) by speculation — the same values, pointer and status as
    sample_walk, bit for bit; r_mean / r_sd size the windows (Sampler.walk_stats)."""
    _dev(random_list, torch.int32, "random_list")
    _dev(pr_dev, torch.int64, "pr_dev")
    _dev(users, torch.int64, "users")
    dev = users.device
    if out is None:
        out = torch.empty(n_batches * batch_keys * num, dtype=torch.int64, device=dev)
    if status is None:
        status = torch.zeros(1, dtype=torch.int32, device=dev)
    bits = reject and used_bits is not None
    wsz = lib().mirec_sample_walk_spec_workspace_size(batch_keys, num, min(n_batches, 16),
                                                      r_mean, r_sd)
    ws = torch.empty(wsz, dtype=torch.uint8, device=dev)
    rc = lib().mirec_sample_walk_spec(
        ptr(random_list), random_list.numel(), ptr(pr_dev), ptr(users), ptr(items), n_batches,
        batch_keys, num, ptr(used_ptr) if reject and not bits else None,
        ptr(used_cols) if reject and not bits else None, ptr(used_bits) if bits else None,
        n_bits if bits else 0, n_key_space, 1 if reject else 0, float(r_mean), float(r_sd),
        ptr(out), out_stride, ptr(user_keys), ptr(item_keys), key_stride, ptr(status), ptr(ws),
        ws.numel(), stream_handle())
    check(rc, "mirec_sample_walk_spec")
    return out


def sample_walk_segments(random_list: torch.Tensor, pr_dev: torch.Tensor, keys: torch.Tensor,
                         seg_ptr: torch.Tensor, max_seg_keys: int, num: int,
                         used_ptr: torch.Tensor | None, used_cols: torch.Tensor | None,
                         n_key_space: int, reject: bool, used_bits: torch.Tensor | None = None,
                         n_bits: int = 0, status: torch.Tensor | None = None) -> torch.Tensor:
    """Successive sample_by_key_ids calls, call s over keys[seg_ptr[s]:seg_ptr[s+1]]
    (device int64 seg_ptr), in one launch; values of call s at seg_ptr[s]*num."""
    _dev(random_list, torch.int32, "random_list")
    _dev(pr_dev, torch.int64, "pr_dev")
    _dev(keys, torch.int64, "keys")
    _dev(seg_ptr, torch.int64, "seg_ptr")
    out = torch.empty(keys.numel() * num, dtype=torch.int64, device=keys.device)
    if status is None:
        status = torch.zeros(1, dtype=torch.int32, device=keys.device)
    bits = reject and used_bits is not None
    if reject and not bits:
        _dev(used_ptr, torch.int64, "used_ptr")
        _dev(used_cols, torch.int32, "used_cols")
    if bits:
        _dev(used_bits, torch.int32, "used_bits")
    ws = torch.empty(lib().mirec_sample_walk_workspace_size(max(max_seg_keys, 1), max(num, 1)),
                     dtype=torch.uint8, device=keys.device)
    rc = lib().mirec_sample_walk_segments(
        ptr(random_list), random_list.numel(), ptr(pr_dev), ptr(keys), ptr(seg_ptr),
        seg_ptr.numel() - 1, max_seg_keys, num,
        ptr(used_ptr) if reject and not bits else None,
        ptr(used_cols) if reject and not bits else None,
        ptr(used_bits) if bits else None, n_bits if bits else 0, n_key_space,
        1 if reject else 0, ptr(out), ptr(status), ptr(ws), ws.numel(), stream_handle())
    check(rc, "mirec_sample_walk_segments")
    return out


def copy_many(dst: list, src: list) -> None:
    """dst[i].copy_(src[i]) for same-size contiguous device tensors, in one launch
    (mirec_copy_many)."""
    n = len(dst)
    if n == 0:
        return
    S = (ctypes.c_void_p * n)()
    D = (ctypes.c_void_p * n)()
    N = (ctypes.c_int64 * n)()
    for i, (d, s) in enumerate(zip(dst, src)):
        if not (d.is_cuda and s.is_cuda and d.is_contiguous() and s.is_contiguous()):
            raise NativeError("copy_many: contiguous device tensors only")
        nb = d.numel() * d.element_size()
        if s.numel() * s.element_size() != nb:
            raise ValueError(f"copy_many: size mismatch at {i}")
        S[i], D[i], N[i] = s.data_ptr(), d.data_ptr(), nb
    check(lib().mirec_copy_many(S, D, N, n, stream_handle()), "mirec_copy_many")


def host_counting_order(keys, key_space: int) -> np.ndarray:
    """Stable sort permutation of integer keys in [0, key_space) (host, O(n))."""
    keys = np.ascontiguousarray(keys, dtype=np.int64)
    order = np.empty(len(keys), dtype=np.int64)
    check(lib().mirec_host_counting_order(keys.ctypes.data, len(keys), int(key_space),
                                          order.ctypes.data), "mirec_host_counting_order")
    return order


def host_csr_build(keys, vals, n_keys: int) -> tuple:
    """(ptr int64[n_keys+1], cols int32) of the distinct (key, value) pairs, each
    row ascending (host, counting pass + per-row sort)."""
    keys = np.ascontiguousarray(keys, dtype=np.int64)
    vals = np.ascontiguousarray(vals, dtype=np.int64)
    ptr = np.empty(int(n_keys) + 1, dtype=np.int64)
    cols = np.empty(max(len(keys), 1), dtype=np.int32)
    nnz = lib().mirec_host_csr_build(keys.ctypes.data, vals.ctypes.data, len(keys), int(n_keys),
                                     ptr.ctypes.data, cols.ctypes.data)
    if nnz < 0:
        check(int(nnz), "mirec_host_csr_build")
    return ptr, cols[:nnz].copy()


def alias_build(counts) -> tuple:
    """Host-side Vose alias table of non-negative integer counts: (thr uint32[n],
    alias int32[n]) numpy arrays (mirec_alias_build)."""
    counts = np.ascontiguousarray(counts, dtype=np.int64)
    n = len(counts)
    thr = np.empty(n, dtype=np.uint32)
    alias = np.empty(n, dtype=np.int32)
    check(lib().mirec_alias_build(counts.ctypes.data, n, thr.ctypes.data, alias.ctypes.data),
          "mirec_alias_build")
    return thr, alias


def sample_alias(thr: torch.Tensor, alias: torch.Tensor, seed: int, counter: int,
                 keys: torch.Tensor, num: int, used_ptr: torch.Tensor | None,
                 used_cols: torch.Tensor | None, n_key_space: int, reject: bool,
                 batch_keys: int | None = None, out: torch.Tensor | None = None,
                 out_stride: int = 0, status: torch.Tensor | None = None,
                 used_bits: torch.Tensor | None = None, n_bits: int = 0) -> torch.Tensor:
    """Alias-table fast-mode draws (NON-PARITY, mirec_sample_alias): `thr` is the
    uint32 threshold table viewed as int32 on the device, `alias` int32."""
    _dev(thr, torch.int32, "thr")
    _dev(alias, torch.int32, "alias")
    _dev(keys, torch.int64, "keys")
    n_keys = keys.numel()
    if batch_keys is None:
        batch_keys = max(n_keys, 1)
    if out is None:
        out = torch.empty(n_keys * num, dtype=torch.int64, device=keys.device)
    if status is None:
        status = torch.zeros(1, dtype=torch.int32, device=keys.device)
    bits = reject and used_bits is not None
    if reject and not bits:
        _dev(used_ptr, torch.int64, "used_ptr")
        _dev(used_cols, torch.int32, "used_cols")
    if bits:
        _dev(used_bits, torch.int32, "used_bits")
    rc = lib().mirec_sample_alias(
        ptr(thr), ptr(alias), thr.numel(), seed & (2 ** 64 - 1), counter, ptr(keys), n_keys,
        batch_keys, num, ptr(used_ptr) if reject and not bits else None,
        ptr(used_cols) if reject and not bits else None, ptr(used_bits) if bits else None,
        n_bits if bits else 0, n_key_space, 1 if reject else 0, ptr(out), out_stride,
        ptr(status), stream_handle())
    check(rc, "mirec_sample_alias")
    return out


def used_bitmap(used_ptr: torch.Tensor, used_cols: torch.Tensor, n_keys: int,
                n_bits: int) -> torch.Tensor:
    """Per-key used-id bitmap [n_keys, ceil(n_bits/32)] (int32 words) of a CSR."""
    _dev(used_ptr, torch.int64, "used_ptr")
    _dev(used_cols, torch.int32, "used_cols")
    words = (n_bits + 31) // 32
    bits = torch.empty(max(n_keys * words, 1), dtype=torch.int32, device=used_ptr.device)
    rc = lib().mirec_used_bitmap_build(ptr(used_ptr), ptr(used_cols), n_keys, n_bits, ptr(bits),
                                       stream_handle())
    check(rc, "mirec_used_bitmap_build")
    return bits


# ---------------------------------------------------------------- K1 gather
def gather_rows(table: torch.Tensor, idx: torch.Tensor, out: torch.Tensor | None = None):
    if not table.is_cuda or not idx.is_cuda:
        raise NativeError("gather_rows: tensors must live on the GPU")
    if not table.is_contiguous():
        raise ValueError("table must be contiguous")
    idx = idx.contiguous()
    row_shape = table.shape[1:]
    if out is None:
        out = torch.empty((idx.numel(),) + tuple(row_shape), dtype=table.dtype,
                          device=table.device)
    row_bytes = table.element_size() * (table[0].numel() if table.dim() > 1 else 1)
    if idx.dtype == torch.int64:
        fn = lib().mirec_gather_rows
    elif idx.dtype == torch.int32:
        fn = lib().mirec_gather_rows_i32idx
    else:
        raise TypeError("idx must be int32 or int64")
    rc = fn(ptr(table), table.shape[0], row_bytes, ptr(idx), idx.numel(), ptr(out),
            stream_handle())
    check(rc, "mirec_gather_rows")
    return out


def window_gather(col: torch.Tensor, start: torch.Tensor, length: torch.Tensor, L: int,
                  out: torch.Tensor | None = None) -> torch.Tensor:
    """out[i, t] = col[start[i] + t] if t < length[i] else 0 (sequence windows)."""
    _dev(start, torch.int64, "start")
    _dev(length, torch.int64, "length")
    if not col.is_cuda or not col.is_contiguous():
        raise NativeError("window_gather: col must be a contiguous GPU tensor")
    n = start.numel()
    if out is None:
        out = torch.empty(n, L, dtype=col.dtype, device=col.device)
    rc = lib().mirec_window_gather(ptr(col), col.element_size(), ptr(start), ptr(length), n, L,
                                   ptr(out), stream_handle())
    check(rc, "mirec_window_gather")
    return out


# ---------------------------------------------------------------- K3 BPR
def bpr_fwd_bwd(EU, EI, user, pos, neg, times: int, gamma: float = 1e-10,
                grad_scale: float | None = None, grads: bool = True, scores: bool = False,
                out: dict | None = None) -> dict:
    """Fused BPR forward/backward on the pairwise layout (bpr.py:74-83, loss.py:47-49)."""
    _dev(EU, torch.float32, "EU")
    _dev(EI, torch.float32, "EI")
    for n_, t_ in (("user", user), ("pos", pos), ("neg", neg)):
        _dev(t_, torch.int64, n_)
    B = user.numel()
    d = EU.shape[1]
    if EI.shape[1] != d or pos.numel() != B or neg.numel() != B * times:
        raise ValueError("bpr_fwd_bwd: inconsistent shapes")
    if grad_scale is None:
        grad_scale = float(torch.tensor(1.0, dtype=torch.float32) /
                           torch.tensor(float(B * times), dtype=torch.float32))
    o = {} if out is None else out
    dev = EU.device
    if "loss_k" not in o:
        o["loss_k"] = torch.empty(B, dtype=torch.float32, device=dev)
    if scores:
        o.setdefault("pos_score", torch.empty(B, dtype=torch.float32, device=dev))
        o.setdefault("neg_score", torch.empty(B * times, dtype=torch.float32, device=dev))
    if grads:
        o.setdefault("gU", torch.empty(B, d, dtype=torch.float32, device=dev))
        o.setdefault("gI", torch.empty((1 + times) * B, d, dtype=torch.float32, device=dev))
    rc = lib().mirec_bpr_fwd_bwd_f32(ptr(EU), EU.shape[0], ptr(EI), EI.shape[0], d, ptr(user),
                                     ptr(pos), ptr(neg), B, times, gamma, grad_scale,
                                     ptr(o["loss_k"]), ptr(o.get("pos_score")),
                                     ptr(o.get("neg_score")), ptr(o.get("gU")),
                                     ptr(o.get("gI")), stream_handle())
    check(rc, "mirec_bpr_fwd_bwd_f32")
    return o


def bpr_fwd_coef(EU, EI, user, pos, neg, times: int, grad_scale: float, gamma: float = 1e-10):
    """K3 forward only: (loss_k [B], coef [times*B]) with coef[r] = d loss / d x_r
    (the data-parallel step's exchanged quantity)."""
    B = user.numel()
    for n_, t_ in (("user", user), ("pos", pos), ("neg", neg)):
        _dev(t_, torch.int64, n_)
    loss_k = torch.empty(B, dtype=torch.float32, device=EU.device)
    coef = torch.empty(max(B * times, 1), dtype=torch.float32, device=EU.device)
    rc = lib().mirec_bpr_fwd_coef_f32(ptr(EU), EU.shape[0], ptr(EI), EI.shape[0], EU.shape[1],
                                      ptr(user), ptr(pos), ptr(neg), B, times, gamma,
                                      grad_scale, ptr(loss_k), ptr(coef), stream_handle())
    check(rc, "mirec_bpr_fwd_coef_f32")
    return loss_k, coef[:B * times]


def bpr_contrib(EU, EI, user, pos, neg, times: int, coef, coef_block: int | None = None,
                coef_stride: int | None = None):
    """Gradient rows (gU [B,d], gI [(1+times)B,d]) of a batch rebuilt from its
    coefficients (mirec_bpr_contrib_f32); default: the single-rank layout."""
    B, d = user.numel(), EU.shape[1]
    _dev(coef, torch.float32, "coef")
    block = B if coef_block is None else coef_block
    stride = times * block if coef_stride is None else coef_stride
    gU = torch.empty(B, d, dtype=torch.float32, device=EU.device)
    gI = torch.empty((1 + times) * B, d, dtype=torch.float32, device=EU.device)
    rc = lib().mirec_bpr_contrib_f32(ptr(EU), EU.shape[0], ptr(EI), EI.shape[0], d, ptr(user),
                                     ptr(pos), ptr(neg), B, times, ptr(coef), block, stride,
                                     ptr(gU), ptr(gI), stream_handle())
    check(rc, "mirec_bpr_contrib_f32")
    return gU, gI


def dot_rows(EU, EI, u, i, out=None):
    """score[r] = <EU[u[r]], EI[i[r]]> (BPR.predict, bpr.py:85-89)."""
    _dev(EU, torch.float32, "EU")
    _dev(EI, torch.float32, "EI")
    u = u.contiguous()
    i = i.contiguous()
    _dev(u, torch.int64, "u")
    _dev(i, torch.int64, "i")
    if out is None:
        out = torch.empty(u.numel(), dtype=torch.float32, device=EU.device)
    rc = lib().mirec_dot_rows_f32(ptr(EU), EU.shape[0], ptr(EI), EI.shape[0], EU.shape[1], ptr(u),
                                  ptr(i), u.numel(), ptr(out), stream_handle())
    check(rc, "mirec_dot_rows_f32")
    return out


def fixed_sum(x: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    _dev(x, torch.float32, "x")
    if out is None:
        out = torch.empty(1, dtype=torch.float32, device=x.device)
    check(lib().mirec_sum_f32(ptr(x), x.numel(), ptr(out), stream_handle()), "mirec_sum_f32")
    return out


# ---------------------------------------------------------------- K2 grouping
class Segments:
    """Grouping of contribution rows by table row (output of K2)."""

    __slots__ = ("perm", "uniq", "seg", "n_uniq", "n", "ws", "pos_seg")

    def __init__(self, n: int, device, ws_bytes: int = 0):
        cap = max(n, 1)
        self.n = n
        self.pos_seg = None      # int32[n]: the segment of each sorted position, if the sort gave it
        self.perm = torch.empty(cap, dtype=torch.int32, device=device)
        self.uniq = torch.empty(cap, dtype=torch.int32, device=device)
        self.seg = torch.empty(cap + 1, dtype=torch.int32, device=device)
        self.n_uniq = torch.empty(1, dtype=torch.int32, device=device)   # every sort writes it
        self.ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=device)


ONESWEEP_MIN = 8193          # above the single-workgroup LDS sort
_SORT_STATUS = {}
_RETIRED = []    # superseded shared scratch buffers: never freed (see _grown)


def _grown(cache, device, n, make, on_capture=None, floor=1 << 16):
    """cache[device]: the device's shared buffer of at least n elements — make(size), size
    at least `floor`, grown on demand. Calls are stream-ordered (the model's stream; a
    graph's warm-up and capture streams wait for each other): every launch on the stream
    finishes with the buffer before the next one starts.

    on_capture: while a graph capture is running a missing or too small buffer is not
    replaced, the caller gets on_capture(n) instead (None: allocate as usual).

    A buffer that is replaced by a larger one stays allocated for the life of the
    process (_RETIRED): a HIP graph captured earlier holds its pointer and replays against
    it, and memory handed back to the caching allocator could be reused for other data,
    so a replay would read garbage look-back words (and scatter outside its outputs). A
    retired status buffer is still zero (every call leaves it so) and only graphs use
    it."""
    key = str(device)
    buf = cache.get(key)
    if buf is None or buf.numel() < n:
        if on_capture is not None and torch.cuda.is_current_stream_capturing():
            return on_capture(n)
        if buf is not None:
            _RETIRED.append(buf)
        buf = cache[key] = make(max(n, floor))
    return buf


def _sort_status(device, words):
    """Zeroed look-back / histogram words of the onesweep sort (every call leaves them
    zero). None while a graph capture is running and the buffer does not exist yet or is
    too small (the caller then takes the radix path)."""
    return _grown(_SORT_STATUS, device, words,
                  lambda m: torch.zeros(m, dtype=torch.int32, device=device),
                  on_capture=lambda n: None)


def segment_sort(keys: torch.Tensor, key_space: int, segs: Segments | None = None) -> Segments:
    _dev(keys, torch.int64, "keys")
    n = keys.numel()
    wsz = lib().mirec_segment_sort_workspace_size(n, key_space)
    if segs is None or segs.n < n or segs.ws.numel() < wsz:
        segs = Segments(n, keys.device, wsz)
    status = None
    if ONESWEEP_MIN <= n < (1 << 30):
        status = _sort_status(keys.device, lib().mirec_segment_sort_onesweep_status_words(n))
    if status is not None:
        if segs.pos_seg is None or segs.pos_seg.numel() < n:
            segs.pos_seg = torch.empty(n, dtype=torch.int32, device=keys.device)
        rc = lib().mirec_segment_sort_onesweep(
            ptr(keys), n, key_space, ptr(segs.perm), ptr(segs.uniq), ptr(segs.seg),
            ptr(segs.n_uniq), ptr(segs.pos_seg), ptr(segs.ws), segs.ws.numel(), ptr(status),
            status.numel(), stream_handle())
        check(rc, "mirec_segment_sort_onesweep")
        return segs
    segs.pos_seg = None
    rc = lib().mirec_segment_sort(ptr(keys), n, key_space, ptr(segs.perm), ptr(segs.uniq),
                                  ptr(segs.seg), ptr(segs.n_uniq), ptr(segs.ws), segs.ws.numel(),
                                  stream_handle())
    check(rc, "mirec_segment_sort")
    return segs


CHAIN_MAX_BLOCK_N, CHAIN_MAX_BLOCKS = 4096, 256


def segment_sort_blocks(keys: torch.Tensor, block_n: int, key_space: int,
                        status: torch.Tensor | None = None) -> Segments:
    """segment_sort for keys in blocks of block_n whose key ranges increase block to
    block (every key of block b below every key of block b+1): same outputs, each
    block sorted in LDS. With `status` (int32, zero, >= n_blocks + 1 entries; left
    zero) and block_n <= 4,096, <= 256 blocks: one launch (mirec_segment_sort_blocks_
    chained); otherwise the sort + concatenation pair (mirec_segment_sort_blocks)."""
    _dev(keys, torch.int64, "keys")
    n = keys.numel()
    nb = -(-n // max(block_n, 1))
    if (status is not None and n > 0 and block_n <= CHAIN_MAX_BLOCK_N
            and nb <= CHAIN_MAX_BLOCKS):
        _dev(status, torch.int32, "status")
        segs = Segments(n, keys.device)
        segs.pos_seg = torch.empty(n, dtype=torch.int32, device=keys.device)
        with timed_launch('k2_blocks'):
            rc = lib().mirec_segment_sort_blocks_chained(
                ptr(keys), n, block_n, key_space, ptr(segs.perm), ptr(segs.uniq), ptr(segs.seg),
                ptr(segs.n_uniq), ptr(status), status.numel(), ptr(segs.pos_seg),
                stream_handle())
        check(rc, "mirec_segment_sort_blocks_chained")
        return segs
    segs = Segments(n, keys.device, lib().mirec_segment_sort_blocks_workspace_size(n, block_n))
    with timed_launch('k2_blocks'):              # two launches: the block sorts, the concat
        rc = lib().mirec_segment_sort_blocks(ptr(keys), n, block_n, key_space, ptr(segs.perm),
                                             ptr(segs.uniq), ptr(segs.seg), ptr(segs.n_uniq),
                                             ptr(segs.ws), segs.ws.numel(), stream_handle())
    check(rc, "mirec_segment_sort_blocks")
    return segs


def segment_sort_fields(cols, offsets, B: int, key_space: int, status: torch.Tensor):
    """DeepFM's token keys (field f: cols[f] + offsets[f], ranges increasing with f) formed
    and grouped in one launch (mirec_segment_sort_fields_chained): (keys [F * B] int64,
    Segments with pos_seg). status: the chained sort's zeroed words (>= F + 1)."""
    nf = len(cols)
    for c in cols:
        _dev(c, torch.int64, "field column")
    _dev(status, torch.int32, "status")
    dev = cols[0].device
    n = nf * B
    keys = torch.empty(n, dtype=torch.int64, device=dev)
    segs = Segments(n, dev)
    segs.pos_seg = torch.empty(n, dtype=torch.int32, device=dev)
    cptr = (ctypes.c_void_p * nf)(*[ptr(c) for c in cols])
    offs = (ctypes.c_int64 * nf)(*[int(o) for o in offsets])
    with timed_launch('k2_blocks'):
        rc = lib().mirec_segment_sort_fields_chained(
            cptr, offs, nf, B, key_space, ptr(keys), ptr(segs.perm), ptr(segs.uniq),
            ptr(segs.seg), ptr(segs.n_uniq), ptr(status), status.numel(), ptr(segs.pos_seg),
            stream_handle())
    check(rc, "mirec_segment_sort_fields_chained")
    return keys, segs


def segment_sort_batched(keys: torch.Tensor, batch_n: int, key_space: int, perm, uniq, seg,
                         n_uniq, ws=None):
    """K2 over consecutive batches of `batch_n` keys, one workgroup per batch."""
    _dev(keys, torch.int64, "keys")
    n = keys.numel()
    nb = max(1, -(-n // max(batch_n, 1)))
    wsz = lib().mirec_segment_sort_workspace_size(nb * batch_n, key_space)
    if ws is None or ws.numel() < wsz:
        ws = torch.empty(wsz, dtype=torch.uint8, device=keys.device)
    rc = lib().mirec_segment_sort_batched(ptr(keys), n, batch_n, key_space, ptr(perm), ptr(uniq),
                                          ptr(seg), ptr(n_uniq), ptr(ws), ws.numel(),
                                          stream_handle())
    check(rc, "mirec_segment_sort_batched")
    return ws


def uniq_ahead_diff(uniq, n_uniq, stride: int, n_batches: int, out, n_out):
    """out[b*stride..] = uniq(b+1) minus uniq(b) (batched segment-sort layout)."""
    for n_, t_ in (("uniq", uniq), ("n_uniq", n_uniq), ("out", out), ("n_out", n_out)):
        _dev(t_, torch.int32, n_)
    rc = lib().mirec_uniq_ahead_diff(ptr(uniq), ptr(n_uniq), stride, n_batches, ptr(out),
                                     ptr(n_out), stream_handle())
    check(rc, "mirec_uniq_ahead_diff")


_SCATTER_WS = {}


def _scatter_ws(device, nbytes):
    """Per-device scratch of the chunked scatter."""
    return _grown(_SCATTER_WS, device, nbytes,
                  lambda m: torch.empty(m, dtype=torch.uint8, device=device))


def _identity_segments(n, uniq, n_uniq, ws, device):
    """Segments over n compact rows, row u = table row uniq[u]: identity perm / seg /
    pos_seg (views of the shared iota: no launch per call)."""
    cap = max(n, 1)
    ident = Segments.__new__(Segments)
    ident.n = n
    iota = _iota(device, cap + 1)
    ident.perm = iota[:cap]
    ident.seg = iota[:cap + 1]
    ident.uniq, ident.n_uniq, ident.ws = uniq, n_uniq, ws
    ident.pos_seg = ident.perm
    return ident


def segment_scatter_add(rows: torch.Tensor, segs: Segments, dense: torch.Tensor) -> torch.Tensor:
    _dev(rows, torch.float32, "rows")
    _dev(dense, torch.float32, "dense")
    d = rows.shape[1]
    wsz = lib().mirec_segment_scatter_add_workspace_size(segs.n, d)
    ws = _scatter_ws(rows.device, wsz)
    rc = lib().mirec_segment_scatter_add_f32(ptr(rows), d, ptr(segs.perm), ptr(segs.uniq),
                                             ptr(segs.seg), ptr(segs.n_uniq), segs.n, ptr(dense),
                                             dense.shape[0], ptr(ws), ws.numel(),
                                             stream_handle())
    check(rc, "mirec_segment_scatter_add_f32")
    return dense


def segment_reduce(rows: torch.Tensor, segs: Segments):
    """(compact [n, d] with row u = sum of segment u's contributions, identity
    Segments over it with the same uniq / n_uniq) — each touched table row's
    gradient as one row for K5."""
    _dev(rows, torch.float32, "rows")
    n, d = segs.n, rows.shape[1]
    out = torch.empty(max(n, 1), d, dtype=torch.float32, device=rows.device)
    ws = _scatter_ws(rows.device, lib().mirec_segment_scatter_add_workspace_size(n, d))
    pos_seg = getattr(segs, 'pos_seg', None)
    if pos_seg is not None and pos_seg is not getattr(segs, 'perm', None):
        rc = lib().mirec_segment_reduce_pos_seg_f32(ptr(rows), d, ptr(segs.perm), ptr(pos_seg),
                                                    ptr(segs.uniq), ptr(segs.seg),
                                                    ptr(segs.n_uniq), n, ptr(out), ptr(ws),
                                                    ws.numel(), stream_handle())
    else:
        rc = lib().mirec_segment_reduce_f32(ptr(rows), d, ptr(segs.perm), ptr(segs.uniq),
                                            ptr(segs.seg), ptr(segs.n_uniq), n, ptr(out),
                                            ptr(ws), ws.numel(), stream_handle())
    check(rc, "mirec_segment_reduce_f32")
    return out, _identity_segments(n, segs.uniq, segs.n_uniq, segs.ws, rows.device)


def segment_merge2(a, b, a_pre=False):
    """Union of two reduced sources of one table — a, b: (compact rows, identity Segments
    with uniq / n_uniq) as segment_reduce returns them — into (rows, identity Segments):
    the second-level segment_reduce of their concatenation, bit for bit, in two launches
    (mirec_segment_merge2_f32). a_pre: a is a previous merge's output."""
    (ra, sa), (rb, sb) = a, b
    _dev(ra, torch.float32, "rows a")
    _dev(rb, torch.float32, "rows b")
    d = ra.shape[1]
    if rb.shape[1] != d:
        raise ValueError("segment_merge2: row widths differ")
    capA, capB = sa.n, sb.n
    cap = max(capA + capB, 1)
    dev = ra.device
    out = torch.empty(cap, d, dtype=torch.float32, device=dev)
    uniq = torch.empty(cap, dtype=torch.int32, device=dev)
    n_uniq = torch.empty(1, dtype=torch.int32, device=dev)
    ws = _scatter_ws(dev, 8 * cap)
    status = _sort_status(dev, cap // 512 + 2)
    if status is None:
        raise NativeError("segment_merge2: no status buffer inside a capture (run one step "
                          "eagerly first)")
    rc = lib().mirec_segment_merge2_f32(ptr(sa.uniq), ptr(sa.n_uniq), capA, ptr(ra),
                                        ptr(sb.uniq), ptr(sb.n_uniq), capB, ptr(rb), d,
                                        1 if a_pre else 0, ptr(uniq), ptr(n_uniq), ptr(out),
                                        ptr(ws), ws.numel(), ptr(status), status.numel(),
                                        stream_handle())
    check(rc, "mirec_segment_merge2_f32")
    return out, _identity_segments(cap, uniq, n_uniq, sa.ws, dev)


def segment_reduce2(rows: torch.Tensor, rows1: torch.Tensor, segs: Segments):
    """segment_reduce of a [n, d] source (2 <= d <= 16) and a [n, 1] source grouped by
    the same segments, in one pass: (compact, compact1, identity Segments), bit for bit
    the two separate reductions."""
    _dev(rows, torch.float32, "rows")
    _dev(rows1, torch.float32, "rows1")
    n, d = segs.n, rows.shape[1]
    out = torch.empty(max(n, 1), d, dtype=torch.float32, device=rows.device)
    out1 = torch.empty(max(n, 1), 1, dtype=torch.float32, device=rows.device)
    ws = _scatter_ws(rows.device, lib().mirec_segment_scatter_add_workspace_size(n, d + 1))
    if getattr(segs, 'pos_seg', None) is not None:     # the chained sort's position -> segment
        rc = lib().mirec_segment_reduce2_pos_seg_f32(
            ptr(rows), d, ptr(rows1), ptr(segs.perm), ptr(segs.pos_seg), ptr(segs.uniq),
            ptr(segs.seg), ptr(segs.n_uniq), n, ptr(out), ptr(out1), ptr(ws), ws.numel(),
            stream_handle())
    else:
        rc = lib().mirec_segment_reduce2_f32(ptr(rows), d, ptr(rows1), ptr(segs.perm),
                                             ptr(segs.uniq), ptr(segs.seg), ptr(segs.n_uniq), n,
                                             ptr(out), ptr(out1), ptr(ws), ws.numel(),
                                             stream_handle())
    check(rc, "mirec_segment_reduce2_f32")
    return out, out1, _identity_segments(n, segs.uniq, segs.n_uniq, segs.ws, rows.device)


_IOTA = {}


def _iota(device, n):
    """0, 1, ..., n-1 as a persistent int32 device tensor (grown on demand; read only).
    Inside a graph capture a size not seen before is graph-pool memory, not cached."""
    def make(m):
        return torch.arange(m, dtype=torch.int32, device=device)
    return _grown(_IOTA, device, n, make, on_capture=make)[:n]


# ---------------------------------------------------------------- K5 Adam
def adam_flat_multi(specs, step_consts, step_idx, beta1=0.9, beta2=0.999, eps=1e-8,
                    weight_decay=0.0, advance_ticket=None):
    """Dense Adam steps of several parameters in one launch per 16 (specs: dicts with
    p, m, v, g — contiguous float32 device tensors of one size each). advance_ticket (an
    int32 [1] device tensor, zero between calls): step_idx is the device step counter and
    the last launch advances it by one after reading it."""
    from recbole_amd._native import FlatParam
    _dev(step_consts, torch.float32, "step_consts")
    _dev(step_idx, torch.int32, "step_idx")
    for i in range(0, len(specs), 16):
        part = specs[i:i + 16]
        arr = (FlatParam * len(part))()
        for t, sp in zip(arr, part):
            for n_ in ("p", "m", "v", "g"):
                x = _dev(sp[n_], torch.float32, n_)
                if not x.is_contiguous() or x.numel() != sp["p"].numel():
                    raise ValueError(f"adam_flat_multi: {n_} must be contiguous, numel of p")
            t.p, t.m, t.v, t.g, t.n = (ptr(sp["p"]), ptr(sp["m"]), ptr(sp["v"]), ptr(sp["g"]),
                                       sp["p"].numel())
        if advance_ticket is not None and i + 16 >= len(specs):
            _dev(advance_ticket, torch.int32, "advance_ticket")
            check(lib().mirec_adam_flat_multi_advance_f32(
                arr, len(part), ptr(step_consts), ptr(step_idx), ptr(advance_ticket), beta1,
                beta2, eps, weight_decay, stream_handle()), "mirec_adam_flat_multi_advance_f32")
            continue
        check(lib().mirec_adam_flat_multi_f32(arr, len(part), ptr(step_consts), ptr(step_idx),
                                              beta1, beta2, eps, weight_decay, stream_handle()),
              "mirec_adam_flat_multi_f32")


def adam_step(p, m, v, step_consts, step_idx, rows=None, segs: Segments | None = None,
              dense_grad=None, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0):
    """One dense Adam step over every row of p (K5); the gradient is the grouped
    compact rows (rows + segs) and/or a dense gradient tensor."""
    for n_, t_ in (("p", p), ("m", m), ("v", v)):
        _dev(t_, torch.float32, n_)
    _dev(step_consts, torch.float32, "step_consts")
    _dev(step_idx, torch.int32, "step_idx")
    if dense_grad is not None:
        _dev(dense_grad, torch.float32, "dense_grad")
    if p.dim() == 2 and p.shape[1] in (16, 32, 64, 128, 256):
        n_rows, d = p.shape
    elif segs is not None:
        raise ValueError("grouped gradients need a 2-D table of width 16..256")
    elif p.numel() % 4 == 0:
        n_rows, d = p.numel() // 4, 4
    else:
        if dense_grad is None:
            raise ValueError("adam_step: a flat parameter needs a dense gradient")
        rc = lib().mirec_adam_flat_f32(ptr(p), ptr(m), ptr(v), p.numel(), ptr(dense_grad),
                                       ptr(step_consts), ptr(step_idx), beta1, beta2, eps,
                                       weight_decay, stream_handle())
        check(rc, "mirec_adam_flat_f32")
        return
    rc = lib().mirec_adam_sparse_grad_f32(
        ptr(p), ptr(m), ptr(v), n_rows, d, ptr(rows),
        ptr(segs.perm) if segs else None, ptr(segs.uniq) if segs else None,
        ptr(segs.seg) if segs else None, ptr(segs.n_uniq) if segs else None,
        segs.n if segs else 0, ptr(dense_grad), ptr(step_consts), ptr(step_idx), beta1, beta2,
        eps, weight_decay, stream_handle())
    check(rc, "mirec_adam_sparse_grad_f32")


ADAM_ZERO_STATE = 0x7fffffff   # MIREC_ADAM_ZERO_STATE (include/mirec.h)


def zero_state_marks(m, v, last, weight_decay=0.0):
    """Set the deferred schedule's step counts for a new window in place:
    last[r] = ADAM_ZERO_STATE where row r's m and v are all +0 (a fixed point of
    the zero-gradient Adam step when weight_decay == 0: flushes and look-aheads
    skip it), else 0."""
    if weight_decay != 0:
        last.zero_()
        return last
    zs = (m.view(torch.int32) == 0).all(1) & (v.view(torch.int32) == 0).all(1)
    last.copy_(torch.where(zs, ADAM_ZERO_STATE, 0).to(torch.int32))
    return last


def reset_marks(last):
    """Window start for counts that already carry zero-state marks: every count
    that is not a mark restarts at 0 (marks stay: those rows are still +0)."""
    last.masked_fill_(last != ADAM_ZERO_STATE, 0)
    return last


def adam_tables(specs):
    """ctypes array of mirec_adam_table from dicts with keys p, m, v (2-D float32
    tables of one width) and optional rows + segs (grouped gradient), dense_grad,
    last (int32 per-row step counts of the deferred schedule), ahead ((rows, count)
    int32 device tensors: rows the next batch reads and this one does not touch,
    completed by the deferred schedule for the next forward pass)."""
    from recbole_amd._native import AdamTable
    arr = (AdamTable * len(specs))()
    for t, s in zip(arr, specs):
        for n_ in ("p", "m", "v"):
            _dev(s[n_], torch.float32, n_)
        t.p, t.m, t.v, t.n_rows = ptr(s["p"]), ptr(s["m"]), ptr(s["v"]), s["p"].shape[0]
        segs = s.get("segs")
        if segs is not None:
            _dev(s["rows"], torch.float32, "rows")
            t.rows, t.perm, t.uniq = ptr(s["rows"]), ptr(segs.perm), ptr(segs.uniq)
            t.seg, t.n_uniq = ptr(segs.seg), ptr(segs.n_uniq)
        if s.get("dense_grad") is not None:
            t.dense_grad = ptr(_dev(s["dense_grad"], torch.float32, "dense_grad"))
        if s.get("last") is not None:
            t.last = ptr(_dev(s["last"], torch.int32, "last"))
        if s.get("ahead") is not None:
            au, an = s["ahead"]
            t.ahead_uniq = ptr(_dev(au, torch.int32, "ahead_uniq"))
            t.ahead_n_uniq = ptr(_dev(an, torch.int32, "ahead_n_uniq"))
        if s.get("p_alt") is not None:            # parity buffer (bpr_adam_step)
            t.p_alt = ptr(_dev(s["p_alt"], torch.float32, "p_alt"))
        if s.get("segs") is None and s.get("grouping") is not None:   # no gradient rows
            g = s["grouping"]
            t.perm, t.uniq, t.seg, t.n_uniq = ptr(g.perm), ptr(g.uniq), ptr(g.seg), ptr(g.n_uniq)
    return arr


def step_records(user_keys, item_keys, n_batches: int, Bc: int, times: int, n_users: int,
                 n_items: int, gu, gi, out=None):
    """K35 records (mirec_step_records) of n_batches batches from their K2 groupings
    gu / gi (Segments or any object with perm, uniq, seg, n_uniq; per-batch strides Bc
    and (1+T)*Bc): (u_rec, u_crec, i_rec, i_crec) int32 device tensors (`out`: the
    caller's four buffers)."""
    for n_, t_ in (("user_keys", user_keys), ("item_keys", item_keys)):
        _dev(t_, torch.int64, n_)
    dev = user_keys.device
    KI = (1 + times) * Bc
    if out is None:
        out = [torch.empty(n_batches * n, dtype=torch.int32, device=dev)
               for n in (step_record_ints(Bc), Bc * 8, step_record_ints(KI), KI * 8)]
    rc = lib().mirec_step_records(ptr(user_keys), ptr(item_keys), n_batches, Bc, times, n_users,
                                  n_items, ptr(gu.perm), ptr(gu.uniq), ptr(gu.seg),
                                  ptr(gu.n_uniq), ptr(gi.perm), ptr(gi.uniq), ptr(gi.seg),
                                  ptr(gi.n_uniq), *[ptr(o) for o in out], None, None, None, None,
                                  stream_handle())
    check(rc, "mirec_step_records")
    return out


def chunk_group(user_keys, item_keys, n_batches: int, Bc: int, times: int, n_users: int,
                n_items: int, outs: dict, records: bool = True, ahead: bool = True):
    """K36 (mirec_chunk_group): the groupings, K35 records and look-ahead lists of a
    chunk in one launch, into the int32 device tensors of `outs` (keys u_perm, u_uniq,
    u_seg, u_nu, i_perm, i_uniq, i_seg, i_nu, and u_rec, u_crec, i_rec, i_crec /
    u_ahead, u_nah, i_ahead, i_nah when asked for). Returns False (nothing launched)
    when the shapes are outside its one-workgroup form."""
    for n_, t_ in (("user_keys", user_keys), ("item_keys", item_keys)):
        _dev(t_, torch.int64, n_)
    names = ["u_perm", "u_uniq", "u_seg", "u_nu", "i_perm", "i_uniq", "i_seg", "i_nu"]
    rec = ["u_rec", "u_crec", "i_rec", "i_crec"]
    ah = ["u_ahead", "u_nah", "i_ahead", "i_nah"]
    args = [ptr(outs[k]) for k in names]
    args += [ptr(outs[k]) for k in rec] if records else [None] * 4
    args += [ptr(outs[k]) for k in ah] if ahead else [None] * 4
    rc = lib().mirec_chunk_group(ptr(user_keys), ptr(item_keys), n_batches, Bc, times, n_users,
                                 n_items, *args, stream_handle())
    if rc < 0:
        check(rc, "mirec_chunk_group")
    return rc == 1


def step_record_ints(per: int) -> int:
    """int32 per batch of one table's K35 record region (mirec_step_record_ints)."""
    n = lib().mirec_step_record_ints(per)
    if n < 0:
        raise ValueError(f"step_record_ints: bad per {per}")
    return n


def step_scratch(Bc: int, times: int, d: int, device):
    """K35 hand-off scratch (u_part, u_join, i_part, i_join): contribution vectors of
    split rows per grouped position, and zeroed arrival counters per row slot and per
    look-ahead slot; reusable by every launch of the same stream (each launch leaves
    the counters zero)."""
    KI = (1 + times) * Bc
    return [torch.empty(Bc * d, dtype=torch.float32, device=device),
            torch.zeros(2 * Bc, dtype=torch.int32, device=device),
            torch.empty(KI * d, dtype=torch.float32, device=device),
            torch.zeros(2 * KI, dtype=torch.int32, device=device)]


def bpr_adam_step(tables, n_max_uniq, d: int, items, Bc: int, times: int, grad_scale: float,
                  loss_k, records, scratch, step_consts, step_base, step_off: int = 0,
                  gamma: float = 1e-10, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0):
    """K35: one training step (BPR forward/backward + the touched rows' deferred Adam
    step + look-ahead) in one launch; tables = adam_tables([users, items]) with p_alt and
    a grouping (n_uniq); records = step_records(...) of this batch; scratch =
    step_scratch(Bc, times, d)."""
    import ctypes
    _dev(items, torch.int64, "items")
    nm = (ctypes.c_int64 * 2)(*n_max_uniq)
    rc = lib().mirec_bpr_adam_step_f32(tables, nm, d, ptr(items), Bc, times, gamma, grad_scale,
                                       ptr(loss_k), *[ptr(r) for r in records],
                                       *[ptr(x) for x in scratch], ptr(step_consts),
                                       ptr(step_base), step_off, beta1, beta2, eps, weight_decay,
                                       stream_handle())
    check(rc, "mirec_bpr_adam_step_f32")


def adam_multi(tables, d: int, step_consts, step_base, step_off: int = 0,
               schedule: str = "streamed", n_max_uniq=None, beta1=0.9, beta2=0.999, eps=1e-8,
               weight_decay=0.0, flush_rows=None):
    """K5 over several tables in one launch: schedule 'streamed' (every row),
    'deferred' (touched rows, replaying skipped zero-gradient steps), 'deferred_pair'
    (two tables, widths d and 1, same semantics, one launch) or 'flush'
    (flush_rows: rows per wave per table, mirec_adam_flush_rows_f32; None = one wave
    per row)."""
    import ctypes
    _dev(step_consts, torch.float32, "step_consts")
    _dev(step_base, torch.int32, "step_base")
    args = (ptr(step_consts), ptr(step_base), step_off, beta1, beta2, eps, weight_decay,
            stream_handle())
    if schedule == "streamed":
        rc = lib().mirec_adam_multi_f32(tables, len(tables), d, *args)
    elif schedule == "deferred":
        nm = (ctypes.c_int64 * len(tables))(*n_max_uniq)
        rc = lib().mirec_adam_deferred_f32(tables, len(tables), nm, d, *args)
    elif schedule == "deferred_pair":          # tables: ([V, d], [V, 1]), one launch
        nm = (ctypes.c_int64 * 2)(*n_max_uniq)
        rc = lib().mirec_adam_deferred_pair_f32(tables, nm, d, *args)
    elif schedule == "flush" and flush_rows is not None:
        rpw = (ctypes.c_int32 * len(tables))(*flush_rows)
        rc = lib().mirec_adam_flush_rows_f32(tables, len(tables), d, rpw, *args)
    elif schedule == "flush":
        rc = lib().mirec_adam_flush_f32(tables, len(tables), d, *args)
    else:
        raise ValueError(f"unknown schedule {schedule!r}")
    check(rc, f"adam_multi[{schedule}]")


_TICKETS = {}


def finish_ticket(device, tag=''):
    """Per-device zeroed int32 of mirec_chunk_finish (tag '') or another kernel's
    last-block ticket (left zero by every launch)."""
    key = (str(device), tag)
    t = _TICKETS.get(key)
    if t is None:
        t = _TICKETS[key] = torch.zeros(1, dtype=torch.int32, device=device)
    return t


def chunk_finish(loss_k, n: int, stride: int, n_steps: int, denom: float, loss_hist, step_base):
    _dev(loss_k, torch.float32, "loss_k")
    _dev(step_base, torch.int32, "step_base")
    rc = lib().mirec_chunk_finish(ptr(loss_k), n, stride, n_steps, float(denom), ptr(loss_hist),
                                  ptr(step_base), ptr(finish_ticket(loss_k.device)),
                                  stream_handle())
    check(rc, "mirec_chunk_finish")


def linear_grad_finish(P, g=None, dW=None):
    """The fixed-order end of a split weight gradient: (sum over c of the partials P[c], db =
    the column sum of g [K, n_out] or None without g), one launch. The sum goes to dW where
    given (dW may be P[0] itself when there is one partial: then only db is formed). One
    partial and no g: P[0], no launch."""
    C = P.shape[0]
    if g is None and C == 1:
        return P[0], None
    dev = P.device
    if dW is None:
        dW = torch.empty(P.shape[1:], dtype=torch.float32, device=dev)
    K = n_out = 0
    db = scratch = ticket = None
    if g is not None:
        K, n_out = g.shape
        db = torch.empty(n_out, dtype=torch.float32, device=dev)
        scratch = torch.empty(max(lib().mirec_linear_grad_finish_scratch(K, n_out), 2),
                              dtype=torch.float32, device=dev)
        ticket = finish_ticket(dev, 'linear')
    check(lib().mirec_linear_grad_finish_f32(ptr(P), C, dW.numel(), ptr(dW), ptr(g), K, n_out,
                                             ptr(db), ptr(scratch), ptr(ticket), stream_handle()),
          "mirec_linear_grad_finish_f32")
    return dW, db


def step_finish(loss_k, denom: float, loss_hist, step_idx):
    _dev(loss_k, torch.float32, "loss_k")
    _dev(step_idx, torch.int32, "step_idx")
    rc = lib().mirec_step_finish(ptr(loss_k), loss_k.numel(), float(denom), ptr(loss_hist),
                                 ptr(step_idx), stream_handle())
    check(rc, "mirec_step_finish")


# ---------------------------------------------------------------- K6 full sort
def fullsort_topk(Uq, EI, K: int, hist_ptr=None, hist_cols=None, pos_ptr=None, pos_cols=None,
                  out: dict | None = None, n_split: int = 1) -> dict:
    _dev(Uq, torch.float32, "Uq")
    _dev(EI, torch.float32, "EI")
    nq, d = Uq.shape
    if EI.shape[1] != d:
        raise ValueError("fullsort_topk: embedding sizes differ")
    for n_, t_, dt in (("hist_ptr", hist_ptr, torch.int64), ("hist_cols", hist_cols, torch.int32),
                       ("pos_ptr", pos_ptr, torch.int64), ("pos_cols", pos_cols, torch.int32)):
        if t_ is not None:
            _dev(t_, dt, n_)
    o = {} if out is None else out
    dev = Uq.device
    o.setdefault("scores", torch.empty(nq, K, dtype=torch.float32, device=dev))
    o.setdefault("ids", torch.empty(nq, K, dtype=torch.int32, device=dev))
    if pos_ptr is not None:
        o.setdefault("pos_flags", torch.empty(nq, K, dtype=torch.uint8, device=dev))
    if n_split > 1:                      # item range split over n_split workgroups + merge
        wsz = lib().mirec_fullsort_topk_split_workspace_size(nq, K, n_split)
        ws = torch.empty(wsz, dtype=torch.uint8, device=dev)
        with timed_launch('fullsort'):
            rc = lib().mirec_fullsort_topk_split_f32(
                ptr(Uq), nq, ptr(EI), EI.shape[0], d, ptr(hist_ptr), ptr(hist_cols),
                ptr(pos_ptr), ptr(pos_cols), K, n_split, ptr(ws), wsz, ptr(o["scores"]),
                ptr(o["ids"]), ptr(o.get("pos_flags")), stream_handle())
        check(rc, "mirec_fullsort_topk_split_f32")
        o["_ws"] = ws
        return o
    with timed_launch('fullsort'):
        rc = lib().mirec_fullsort_topk_f32(ptr(Uq), nq, ptr(EI), EI.shape[0], d, ptr(hist_ptr),
                                           ptr(hist_cols), ptr(pos_ptr), ptr(pos_cols), K,
                                           ptr(o["scores"]), ptr(o["ids"]),
                                           ptr(o.get("pos_flags")), stream_handle())
    check(rc, "mirec_fullsort_topk_f32")
    return o


def score_matrix(Uq, EI, out=None):
    _dev(Uq, torch.float32, "Uq")
    _dev(EI, torch.float32, "EI")
    if out is None:
        out = torch.empty(Uq.shape[0], EI.shape[0], dtype=torch.float32, device=Uq.device)
    rc = lib().mirec_score_matrix_f32(ptr(Uq), Uq.shape[0], ptr(EI), EI.shape[0], Uq.shape[1],
                                      ptr(out), stream_handle())
    check(rc, "mirec_score_matrix_f32")
    return out


# ---------------------------------------------------------------- K14 NeuMF
def neumf_gather(user, item, U_mf, I_mf, w_mf, U_mlp, I_mlp):
    """K14a: x [B, 2 dm] = [U_mlp[u] | I_mlp[i]] (None when the MLP tables are None) and
    z_mf [B] = sum_k w_mf[k] U_mf[u, k] I_mf[i, k] (zeros when the MF tables are None)."""
    user, item = _dev(user, torch.int64, "user"), _dev(item, torch.int64, "item")
    B, dev = user.numel(), user.device
    mf, mlp = U_mf is not None, U_mlp is not None
    n_users = (U_mf if mf else U_mlp).shape[0]
    n_items = (I_mf if mf else I_mlp).shape[0]
    for n_, t_ in (("U_mf", U_mf), ("I_mf", I_mf), ("w_mf", w_mf), ("U_mlp", U_mlp),
                   ("I_mlp", I_mlp)):
        if t_ is not None:
            _dev(t_, torch.float32, n_)
    dmf = U_mf.shape[1] if mf else 0
    dm = U_mlp.shape[1] if mlp else 0
    x = torch.empty(B, 2 * dm, dtype=torch.float32, device=dev) if mlp else None
    z = torch.empty(B, dtype=torch.float32, device=dev)
    with timed_launch('neumf_gather'):
        rc = lib().mirec_neumf_gather_f32(ptr(user), ptr(item), B, ptr(U_mf), ptr(I_mf), dmf,
                                          ptr(w_mf), ptr(U_mlp), ptr(I_mlp), dm, n_users,
                                          n_items, ptr(x), ptr(z), stream_handle())
    check(rc, "mirec_neumf_gather_f32")
    return x, z


def neumf_gather_bwd(user, item, U_mf, I_mf, w_mf, g, gx, n_users: int, n_items: int):
    """K14b: per-row gradients (gU_mf, gI_mf, gU_mlp, gI_mlp) and dw_mf; g None skips the
    MF half, gx None the MLP half."""
    B, dev = user.numel(), user.device
    mf, mlp = g is not None, gx is not None
    E = lambda *sh: torch.empty(*sh, dtype=torch.float32, device=dev)
    dmf = U_mf.shape[1] if mf else 0
    dm = gx.shape[1] // 2 if mlp else 0
    gU_mf, gI_mf, dw = (E(B, dmf), E(B, dmf), E(dmf)) if mf else (None, None, None)
    gU_mlp, gI_mlp = (E(B, dm), E(B, dm)) if mlp else (None, None)
    if mf:
        g = _dev(g, torch.float32, "g")
    if mlp:
        gx = _dev(gx, torch.float32, "gx")
    with timed_launch('neumf_gather_bwd'):
        rc = lib().mirec_neumf_gather_bwd_f32(
            ptr(user), ptr(item), B, ptr(U_mf) if mf else None, ptr(I_mf) if mf else None, dmf,
            ptr(w_mf) if mf else None, ptr(g), ptr(gx), dm, n_users, n_items, ptr(gU_mf),
            ptr(gI_mf), ptr(gU_mlp), ptr(gI_mlp), ptr(dw), stream_handle())
    check(rc, "mirec_neumf_gather_bwd_f32")
    return gU_mf, gI_mf, gU_mlp, gI_mlp, dw


def neumf_project(table, W, col0: int, bias=None, idx=None):
    """out [n, H] = bias + table[rows] @ W[:, col0:col0 + dm].T (rows = idx, or every row):
    the user part A / item part Bm of the first MLP layer for K14c."""
    _dev(table, torch.float32, "table")
    _dev(W, torch.float32, "W")
    n = table.shape[0] if idx is None else idx.numel()
    if idx is not None:
        idx = _dev(idx, torch.int64, "idx")
    out = torch.empty(n, W.shape[0], dtype=torch.float32, device=table.device)
    rc = lib().mirec_neumf_project_f32(ptr(table), ptr(idx), n, table.shape[0], table.shape[1],
                                       ptr(W), W.shape[1], col0, ptr(bias), W.shape[0], ptr(out),
                                       stream_handle())
    check(rc, "mirec_neumf_project_f32")
    return out


def pair_mlp_desc(weights, biases, w_h, bias, dmf: int):
    """struct mirec_pair_mlp for hidden layers 2..L (weights[l] [H_l, H_{l-1}], l >= 1;
    weights[0] only gives H_1) and the head (w_h [H_L], bias: a 1-element tensor or None).
    Returns (descriptor, tensors it points at)."""
    from recbole_amd._native import PairMlpDesc
    d = PairMlpDesc()
    d.n_hidden = len(weights)
    keep = []
    for l, w in enumerate(weights[:4]):
        d.H[l] = w.shape[0]
        if l >= 1:
            w = _dev(w, torch.float32, "weight")
            d.W[l] = ptr(w)
            d.b[l] = ptr(biases[l])
            keep += [w, biases[l]]
    d.dmf = dmf
    d.w_h, d.bias = ptr(w_h), ptr(bias)
    keep += [w_h, bias]
    return d, keep


def pair_mlp_supported(widths, dmf: int) -> bool:
    """K14c's shapes: 2..4 hidden layers of widths that are multiples of 16 in 16..256,
    dmf a multiple of 4 up to 128 (0: no MF term), and an LDS layout that fits."""
    from recbole_amd._native import PairMlpDesc
    if not 2 <= len(widths) <= 4:
        return False
    d = PairMlpDesc()
    d.n_hidden = len(widths)
    for l, h in enumerate(widths):
        d.H[l] = h
    d.dmf = dmf
    for l in range(1, len(widths)):            # non-NULL, aligned: shapes only are judged
        d.W[l] = 16
    d.w_h = 16
    return lib().mirec_pair_mlp_supported(ctypes.byref(d)) == 1


def pair_mlp_topk(desc, A, Pq, Bm, I_mf, K: int, hist_ptr=None, hist_cols=None, pos_ptr=None,
                  pos_cols=None, out: dict | None = None) -> dict:
    """K14c, top-K mode: fullsort_topk's outputs ('scores' = logits, 'ids', 'pos_flags')."""
    _dev(A, torch.float32, "A")
    _dev(Bm, torch.float32, "Bm")
    for n_, t_, dt in (("hist_ptr", hist_ptr, torch.int64), ("hist_cols", hist_cols, torch.int32),
                       ("pos_ptr", pos_ptr, torch.int64), ("pos_cols", pos_cols, torch.int32),
                       ("Pq", Pq, torch.float32), ("I_mf", I_mf, torch.float32)):
        if t_ is not None:
            _dev(t_, dt, n_)
    nq, dev = A.shape[0], A.device
    o = {} if out is None else out
    o.setdefault("scores", torch.empty(nq, K, dtype=torch.float32, device=dev))
    o.setdefault("ids", torch.empty(nq, K, dtype=torch.int32, device=dev))
    if pos_ptr is not None:
        o.setdefault("pos_flags", torch.empty(nq, K, dtype=torch.uint8, device=dev))
    with timed_launch('pair_mlp'):
        rc = lib().mirec_pair_mlp_f32(ctypes.byref(desc), ptr(A), ptr(Pq), nq, ptr(Bm), ptr(I_mf),
                                      Bm.shape[0], ptr(hist_ptr), ptr(hist_cols), ptr(pos_ptr),
                                      ptr(pos_cols), K, ptr(o["scores"]), ptr(o["ids"]),
                                      ptr(o.get("pos_flags")), None, stream_handle())
    check(rc, "mirec_pair_mlp_f32")
    return o


def pair_mlp_scores(desc, A, Pq, Bm, I_mf, out=None):
    """K14c, scores mode: the [nq, I] logits (no mask, no top-K)."""
    _dev(A, torch.float32, "A")
    _dev(Bm, torch.float32, "Bm")
    if out is None:
        out = torch.empty(A.shape[0], Bm.shape[0], dtype=torch.float32, device=A.device)
    with timed_launch('pair_mlp'):
        rc = lib().mirec_pair_mlp_f32(ctypes.byref(desc), ptr(A), ptr(Pq), A.shape[0], ptr(Bm),
                                      ptr(I_mf), Bm.shape[0], None, None, None, None, 1, None,
                                      None, None, ptr(out), stream_handle())
    check(rc, "mirec_pair_mlp_f32")
    return out


# ---------------------------------------------------------------- K15 sparse user rows
BAG_ROW_SPLIT = 64       # MIREC_BAG_ROW_SPLIT (include/mirec.h): items per K15a unit
BAG_SEG_CHUNK = 32       # MIREC_BAG_SEG_CHUNK: sorted positions per K15b wave


def _hist(users, hist_ptr, hist_cols):
    _dev(users, torch.int64, "users")
    _dev(hist_ptr, torch.int64, "hist_ptr")
    _dev(hist_cols, torch.int32, "hist_cols")
    return hist_ptr.numel() - 1


def colsum(x, out=None):
    """out[j] = sum_i x[i, j] in row order (mirec_colsum_f32: fixed order, bias gradients)."""
    _dev(x, torch.float32, "x")
    n, m = x.shape
    if out is None:
        out = torch.empty(m, dtype=torch.float32, device=x.device)
    check(lib().mirec_colsum_f32(ptr(x), n, m, ptr(out), stream_handle()), "mirec_colsum_f32")
    return out


def bag_linear_fwd(users, hist_ptr, hist_cols, Wt, bias, p: float = 0.0, rng=None,
                   train: bool = False, tanh: bool = False, drawn=None):
    """K15a: y [B, N] = act(bias + c_b * sum of the kept rows Wt[i], i in the history set of
    users[b]); Wt [n_items, N] item-major, N a multiple of 4 in 4..1024. With train and
    0 < p < 1, rng = (seed, device int64 counter) keys the draw and `drawn` (device int64
    [1]) receives the counter value used."""
    n_users = _hist(users, hist_ptr, hist_cols)
    _dev(Wt, torch.float32, "Wt")
    _dev(bias, torch.float32, "bias")
    n_items, N = Wt.shape
    B = users.numel()
    drop = bool(train) and p > 0
    seed, counter = rng if drop else (0, None)
    y = torch.empty(B, N, dtype=torch.float32, device=Wt.device)
    with timed_launch('bag_fwd'):
        rc = lib().mirec_bag_linear_fwd_f32(ptr(users), B, ptr(hist_ptr), ptr(hist_cols), n_users,
                                            n_items, ptr(Wt), ptr(bias), N, float(p), seed,
                                            ptr(counter), ptr(drawn), int(drop), int(bool(tanh)),
                                            ptr(y), stream_handle())
    check(rc, "mirec_bag_linear_fwd_f32")
    return y


def bag_row_offsets(users, hist_ptr):
    """(off int64 [B + 1], nnz): the exclusive prefix sums of the batch rows' lengths and
    their total — the ONE host read of a K15 step (it sizes the K15b launches)."""
    lens = hist_ptr[users + 1] - hist_ptr[users]
    off = torch.zeros(users.numel() + 1, dtype=torch.int64, device=users.device)
    torch.cumsum(lens, 0, out=off[1:])
    return off, int(off[-1].item())


def bag_linear_bwd(G, users, hist_ptr, hist_cols, n_items: int, p: float = 0.0, rng=None,
                   train: bool = False, drawn=None, offsets=None):
    """K15b: the dense dWt [n_items, N] of K15a for G [B, N], the gradient at the
    pre-activation: expand the batch's nonzeros (the forward's draw recomputed from
    `drawn`, the counter advanced), group them by item (K2, stable) and sum
    weight * G[row] through the permutation, ascending batch row. Every row is written."""
    n_users = _hist(users, hist_ptr, hist_cols)
    _dev(G, torch.float32, "G")
    B, N = G.shape
    dev = G.device
    off, nnz = offsets if offsets is not None else bag_row_offsets(users, hist_ptr)
    drop = bool(train) and p > 0
    seed, counter = rng if drop else (0, None)
    keys = torch.empty(max(nnz, 1), dtype=torch.int64, device=dev)
    row_of = torch.empty(max(nnz, 1), dtype=torch.int32, device=dev)
    wgt = torch.empty(max(nnz, 1), dtype=torch.float32, device=dev)
    rc = lib().mirec_bag_expand_f32(ptr(users), B, ptr(hist_ptr), ptr(hist_cols), n_users,
                                    n_items, ptr(off), nnz, float(p), seed, ptr(drawn),
                                    ptr(counter), int(drop), ptr(keys), ptr(row_of), ptr(wgt),
                                    stream_handle())
    check(rc, "mirec_bag_expand_f32")
    dWt = torch.empty(n_items, N, dtype=torch.float32, device=dev)       # every row written
    perm, ws, wsz = None, None, 0
    if nnz > 0:
        segs = segment_sort(keys[:nnz], n_items)
        perm = segs.perm
        wsz = lib().mirec_bag_linear_bwd_workspace_size(nnz, N)
        ws = torch.empty(wsz, dtype=torch.uint8, device=dev)
    with timed_launch('bag_bwd'):
        rc = lib().mirec_bag_linear_bwd_f32(ptr(G), B, N, nnz, ptr(keys), ptr(row_of), ptr(wgt),
                                            ptr(perm), n_items, ptr(dWt), ptr(ws), wsz,
                                            stream_handle())
    check(rc, "mirec_bag_linear_bwd_f32")
    return dWt


def _logits_ld(z):
    """Row stride of a float32 [B, I] device matrix whose rows are contiguous."""
    if not isinstance(z, torch.Tensor):
        raise TypeError("the matrix must be a torch.Tensor")
    if not z.is_cuda:
        raise NativeError(f"the matrix must live on the GPU (got {z.device}); no CPU fallback "
                          "exists")
    if z.dtype != torch.float32 or z.dim() != 2 or z.stride(1) != 1 or z.stride(0) < z.shape[1]:
        raise ValueError("the matrix must be float32 [B, I] with unit column stride and row "
                         "stride >= I")
    return z.stride(0)


def multinomial_nll_fwd(z, users, hist_ptr, hist_cols):
    """K15c forward: (lse [B], loss_rows [B], stat [B, 2]) of the stored logits z [B, I] (a
    row-strided view is taken as it is); loss_rows[b] = n_b lse[b] - sum of z[b, i] over the
    history set, stat[b] = the row's (max, sum of exp(z - max)), which the backward reads."""
    n_users = _hist(users, hist_ptr, hist_cols)
    ld = _logits_ld(z)
    B, I = z.shape
    lse = torch.empty(B, dtype=torch.float32, device=z.device)
    stat = torch.empty(B, 2, dtype=torch.float32, device=z.device)
    loss_rows = torch.empty(B, dtype=torch.float32, device=z.device)
    rc = lib().mirec_multinomial_nll_fwd_f32(ptr(z), ld, B, I, ptr(users), ptr(hist_ptr),
                                             ptr(hist_cols), n_users, ptr(lse), ptr(stat),
                                             ptr(loss_rows), stream_handle())
    check(rc, "mirec_multinomial_nll_fwd_f32")
    return lse, loss_rows, stat


def multinomial_nll_bwd_(z, users, hist_ptr, hist_cols, stat, g):
    """K15c backward, IN PLACE: z[b, i] <- (n_b softmax(z[b])[i] - [i in the set]) g / B, from
    the forward's stat; g a one-element device tensor (no host sync). Returns z."""
    n_users = _hist(users, hist_ptr, hist_cols)
    ld = _logits_ld(z)
    _dev(stat, torch.float32, "stat")
    _dev(g, torch.float32, "g")
    B, I = z.shape
    if stat.numel() != 2 * B or g.numel() != 1:
        raise ValueError("multinomial_nll_bwd_: shapes differ")
    rc = lib().mirec_multinomial_nll_bwd_f32(ptr(z), ld, B, I, ptr(users), ptr(hist_ptr),
                                             ptr(hist_cols), n_users, ptr(stat), ptr(g),
                                             stream_handle())
    check(rc, "mirec_multinomial_nll_bwd_f32")
    return z


def matrix_topk(scores, K: int, hist_ptr=None, hist_cols=None, pos_ptr=None, pos_cols=None,
                out: dict | None = None) -> dict:
    """K15d: fullsort_topk's outputs for a GIVEN score matrix [nq, I] (a row-strided view is
    taken as it is): item 0 and the history masked, (score desc, id asc), 1 <= K <= 50."""
    ld = _logits_ld(scores)
    for n_, t_, dt in (("hist_ptr", hist_ptr, torch.int64), ("hist_cols", hist_cols, torch.int32),
                       ("pos_ptr", pos_ptr, torch.int64), ("pos_cols", pos_cols, torch.int32)):
        if t_ is not None:
            _dev(t_, dt, n_)
    nq, I = scores.shape
    o = {} if out is None else out
    dev = scores.device
    o.setdefault("scores", torch.empty(nq, K, dtype=torch.float32, device=dev))
    o.setdefault("ids", torch.empty(nq, K, dtype=torch.int32, device=dev))
    if pos_ptr is not None:
        o.setdefault("pos_flags", torch.empty(nq, K, dtype=torch.uint8, device=dev))
    with timed_launch('matrix_topk'):
        rc = lib().mirec_matrix_topk_f32(ptr(scores), nq, I, ld, ptr(hist_ptr), ptr(hist_cols),
                                         ptr(pos_ptr), ptr(pos_cols), K, ptr(o["scores"]),
                                         ptr(o["ids"]), ptr(o.get("pos_flags")), stream_handle())
    check(rc, "mirec_matrix_topk_f32")
    return o


# ---------------------------------------------------------------- K12 full-catalogue CE
def full_ce_splits(B: int, I: int, d: int, splits: int = 0) -> int:
    """The item split K12 uses for `splits` (0 = auto): a host-side pure function."""
    return int(lib().mirec_full_ce_splits(B, I, d, splits))


def _full_ce_ws(S, E, splits):
    n = lib().mirec_full_ce_workspace_size(S.shape[0], E.shape[0], S.shape[1], splits)
    return torch.empty(n, dtype=torch.uint8, device=S.device)


def full_ce_fwd(S, E, target, splits: int = 0):
    """K12a: (lse[B], loss_rows[B]) of the logits S @ E^T against `target`, without the
    [B, I] matrix; loss_rows = lse - logit of the target."""
    _dev(S, torch.float32, "S")
    _dev(E, torch.float32, "E")
    _dev(target, torch.int64, "target")
    B, d = S.shape
    if E.shape[1] != d or target.numel() != B:
        raise ValueError("full_ce_fwd: shapes differ")
    lse = torch.empty(B, dtype=torch.float32, device=S.device)
    loss_rows = torch.empty(B, dtype=torch.float32, device=S.device)
    ws = _full_ce_ws(S, E, splits)
    rc = lib().mirec_full_ce_fwd_f32(ptr(S), B, ptr(E), E.shape[0], d, ptr(target), splits,
                                     ptr(lse), ptr(loss_rows), ptr(ws), stream_handle())
    check(rc, "mirec_full_ce_fwd_f32")
    return lse, loss_rows


def full_ce_bwd(S, E, target, lse, g, splits: int = 0):
    """K12b + K12c: (gS[B, d], dE[I, d]) of the mean cross entropy for the incoming
    gradient `g`, a one-element device tensor (read on the device: no host sync)."""
    _dev(S, torch.float32, "S")
    _dev(E, torch.float32, "E")
    _dev(target, torch.int64, "target")
    _dev(lse, torch.float32, "lse")
    _dev(g, torch.float32, "g")
    B, d = S.shape
    if E.shape[1] != d or target.numel() != B or lse.numel() != B or g.numel() != 1:
        raise ValueError("full_ce_bwd: shapes differ")
    gS = torch.empty(B, d, dtype=torch.float32, device=S.device)
    dE = torch.empty(E.shape[0], d, dtype=torch.float32, device=S.device)   # every row written
    ws = _full_ce_ws(S, E, splits)
    rc = lib().mirec_full_ce_bwd_f32(ptr(S), B, ptr(E), E.shape[0], d, ptr(target), ptr(lse),
                                     ptr(g), splits, ptr(gS), ptr(dE), ptr(ws), stream_handle())
    check(rc, "mirec_full_ce_bwd_f32")
    return gS, dE


def _rows_ce_args(X, row, n_rows, E, target, what):
    _dev(X, torch.float32, "X")
    _dev(row, torch.int64, "row")
    _dev(E, torch.float32, "E")
    _dev(target, torch.int64, "target")
    if n_rows is not None:
        _dev(n_rows, torch.int32, "n_rows")
    R, d = row.numel(), X.shape[1]
    if X.dim() != 2 or E.shape[1] != d or target.numel() != R or (
            n_rows is not None and n_rows.numel() != 1):
        raise ValueError(f"{what}: shapes differ")
    return R, d


def full_ce_rows_fwd(X, row, target, E, n_rows=None, splits: int = 0):
    """K12a over gathered rows (K17): (lse[R], loss_rows[R]) of the logits X[row] @ E^T against
    `target`; only the first min(R, n_rows[0]) queries exist (n_rows: a one-element int32
    device tensor, None = all R), later entries are exactly 0. row[r] of an existing query
    must lie in [0, X.shape[0]) (not checked: no host sync)."""
    R, d = _rows_ce_args(X, row, n_rows, E, target, "full_ce_rows_fwd")
    lse = torch.empty(R, dtype=torch.float32, device=X.device)
    loss_rows = torch.empty(R, dtype=torch.float32, device=X.device)
    n = lib().mirec_full_ce_workspace_size(R, E.shape[0], d, splits)
    ws = torch.empty(n, dtype=torch.uint8, device=X.device)
    rc = lib().mirec_rows_ce_fwd_f32(ptr(X), X.shape[0], ptr(row), R, ptr(n_rows), ptr(E),
                                     E.shape[0], d, ptr(target), splits, ptr(lse),
                                     ptr(loss_rows), ptr(ws), stream_handle())
    check(rc, "mirec_rows_ce_fwd_f32")
    return lse, loss_rows


def full_ce_rows_bwd(X, row, target, E, lse, g, n_rows=None, splits: int = 0, dE=None):
    """K12b + K12c over gathered rows (K17): (gS[R, d] compact, dE[I, d]) with the factor
    g[0] as it stands (the caller folds 1 / count in; no division by R); gS rows past the
    count are exactly 0. dE: an [I, d] tensor to write into (e.g. the first rows of a larger
    table gradient), allocated when None."""
    R, d = _rows_ce_args(X, row, n_rows, E, target, "full_ce_rows_bwd")
    _dev(lse, torch.float32, "lse")
    _dev(g, torch.float32, "g")
    if lse.numel() != R or g.numel() != 1:
        raise ValueError("full_ce_rows_bwd: shapes differ")
    gS = torch.empty(R, d, dtype=torch.float32, device=X.device)
    if dE is None:                                                # every row written
        dE = torch.empty(E.shape[0], d, dtype=torch.float32, device=X.device)
    elif _dev(dE, torch.float32, "dE").shape != E.shape:
        raise ValueError("full_ce_rows_bwd: dE must have E's shape")
    n = lib().mirec_full_ce_workspace_size(R, E.shape[0], d, splits)
    ws = torch.empty(n, dtype=torch.uint8, device=X.device)
    rc = lib().mirec_rows_ce_bwd_f32(ptr(X), X.shape[0], ptr(row), R, ptr(n_rows), ptr(E),
                                     E.shape[0], d, ptr(target), ptr(lse), ptr(g), splits,
                                     ptr(gS), ptr(dE), ptr(ws), stream_handle())
    check(rc, "mirec_rows_ce_bwd_f32")
    return gS, dE


# ---------------------------------------------------------------- K17 Cloze task (BERT4Rec)
def cloze_mask(item_seq, M: int, n_items: int, mask_ratio: float, seed: int, counter,
               negatives: bool = True):
    """K17a: (masked_seq[B, L], pos_items[B, M], neg_items[B, M] or None, masked_index[B, M])
    of BERT4Rec.reconstruct_train_data, drawn on the device from (seed, counter[0]). The
    counter is only read: the caller advances it (counter.add_(1)) after the call."""
    _dev(item_seq, torch.int64, "item_seq")
    _dev(counter, torch.int64, "counter")
    if item_seq.dim() != 2:
        raise ValueError("cloze_mask: item_seq must be [B, L]")
    B, L = item_seq.shape
    if n_items - 1 <= L:
        raise ValueError(f"cloze_mask: n_items - 1 = {n_items - 1} <= L = {L}: a negative "
                         f"outside the row could not be drawn")
    if not (1 <= M <= L <= 64):
        raise ValueError(f"cloze_mask: needs 1 <= M <= L <= 64, got M = {M}, L = {L}")
    dev = item_seq.device
    masked_seq = torch.empty(B, L, dtype=torch.int64, device=dev)
    pos = torch.empty(B, M, dtype=torch.int64, device=dev)
    idx = torch.empty(B, M, dtype=torch.int64, device=dev)
    neg = torch.empty(B, M, dtype=torch.int64, device=dev) if negatives else None
    rc = lib().mirec_cloze_mask(ptr(item_seq), B, L, M, n_items, float(mask_ratio),
                                seed & ((1 << 64) - 1), ptr(counter), ptr(masked_seq), ptr(pos),
                                ptr(idx), ptr(neg), stream_handle())
    check(rc, "mirec_cloze_mask")
    return masked_seq, pos, neg, idx


def cloze_compact(masked_index, pos_items, L: int):
    """K17b: (act_row[B*M], act_target[B*M], n_act[1] int32, slot_of[B*L] int32): the slots
    with masked_index > 0 in ascending (b, slot) order as rows b*L + index of the [B*L, d]
    encoder output, and the inverse map (-1 elsewhere). One launch, no host sync."""
    _dev(masked_index, torch.int64, "masked_index")
    _dev(pos_items, torch.int64, "pos_items")
    if masked_index.dim() != 2 or pos_items.shape != masked_index.shape:
        raise ValueError("cloze_compact: masked_index and pos_items must be [B, M]")
    B, M = masked_index.shape
    dev = masked_index.device
    act_row = torch.empty(B * M, dtype=torch.int64, device=dev)
    act_target = torch.empty(B * M, dtype=torch.int64, device=dev)
    n_act = torch.empty(1, dtype=torch.int32, device=dev)
    slot_of = torch.empty(B * L, dtype=torch.int32, device=dev)
    rc = lib().mirec_cloze_compact(ptr(masked_index), ptr(pos_items), B, L, M, ptr(act_row),
                                   ptr(act_target), ptr(n_act), ptr(slot_of), stream_handle())
    check(rc, "mirec_cloze_compact")
    return act_row, act_target, n_act, slot_of


def rows_from_slots(gS, slot_of):
    """K17c: gX[p] = gS[slot_of[p]] where slot_of[p] >= 0, zeros elsewhere; [n_pos, d], every
    element written once."""
    _dev(gS, torch.float32, "gS")
    _dev(slot_of, torch.int32, "slot_of")
    if gS.dim() != 2:
        raise ValueError("rows_from_slots: gS must be [R, d]")
    n, d = slot_of.numel(), gS.shape[1]
    gX = torch.empty(n, d, dtype=torch.float32, device=gS.device)
    rc = lib().mirec_rows_from_slots_f32(ptr(gS), ptr(slot_of), n, d, ptr(gX), stream_handle())
    check(rc, "mirec_rows_from_slots_f32")
    return gX


# ---------------------------------------------------------------- K7 graph propagation
def _rows_ref(t):
    """mirec_rows_ref from None, a [n, d] tensor, or a (lo, hi) pair of row blocks."""
    from recbole_amd._native import RowsRef
    if t is None:
        return RowsRef(None, None, 0)
    if isinstance(t, tuple):
        lo, hi = t
        _dev(lo, torch.float32, "rows.lo")
        _dev(hi, torch.float32, "rows.hi")
        return RowsRef(ptr(lo), ptr(hi), lo.shape[0])
    _dev(t, torch.float32, "rows")
    return RowsRef(ptr(t), None, t.shape[0])


def _rows_n(t):
    if t is None:
        return None
    if isinstance(t, tuple):
        return t[0].shape[0] + t[1].shape[0], t[0].shape[1]
    return t.shape[0], t.shape[1]


class SpmmPlan:
    """Device CSR of a square sparse matrix plus the K7 load-balancing plan:
    every row is cut into units of at most `piece` nonzeros (include/mirec.h)."""

    def __init__(self, row_ptr: np.ndarray, cols: np.ndarray, vals: np.ndarray, device,
                 piece: int = 256, max_units: int = 1024):
        row_ptr = np.asarray(row_ptr, dtype=np.int64)
        n = len(row_ptr) - 1
        deg = np.diff(row_ptr)
        # hub rows (a Zipf head item has millions of edges) are cut into at most
        # max_units units so the fixup of their partials stays short
        n_units_row = np.minimum(np.maximum(1, -(-deg // piece)), max_units)
        first_unit = np.concatenate([[0], np.cumsum(n_units_row)])
        n_units = int(first_unit[-1])
        unit_row = np.repeat(np.arange(n, dtype=np.int32), n_units_row)
        k_in_row = np.arange(n_units, dtype=np.int64) - first_unit[:-1][unit_row]
        # near-equal split of row r's deg nonzeros over its units
        unit_beg = row_ptr[:-1][unit_row] + (k_in_row * deg[unit_row]) // n_units_row[unit_row]
        unit_beg = np.concatenate([unit_beg, [row_ptr[-1]]])
        split = n_units_row > 1
        unit_slot = np.full(n_units, -1, dtype=np.int32)
        in_split = split[unit_row]
        unit_slot[in_split] = np.arange(int(in_split.sum()), dtype=np.int32)
        fix_row = np.nonzero(split)[0].astype(np.int32)
        fix_ptr = np.concatenate([[0], np.cumsum(n_units_row[split])]).astype(np.int32)
        self.n_rows, self.nnz, self.piece = n, int(row_ptr[-1]), piece
        self.n_units, self.n_fix, self.n_slots = n_units, len(fix_row), int(fix_ptr[-1])
        T = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=device)
        self.row_ptr, self.cols, self.vals = T(row_ptr), T(cols.astype(np.int32)), \
            T(vals.astype(np.float32))
        self.unit_row, self.unit_beg, self.unit_slot = T(unit_row), T(unit_beg), T(unit_slot)
        self.fix_row, self.fix_ptr = T(fix_row), T(fix_ptr)
        self._partial = {}

    def partial(self, d, device):
        if self.n_slots == 0:
            return None
        if d not in self._partial:
            self._partial[d] = torch.empty(self.n_slots, d, dtype=torch.float32, device=device)
        return self._partial[d]


def spmm_csr(plan: SpmmPlan, x, y=None, add=None, add_scale: float = 1.0, acc_in=None,
             acc_out=None, acc_scale: float = 1.0, vals=None):
    """One K7 launch: y = A @ x (+ add_scale*add); Y = y; ACC_OUT = (ACC_IN + y)*acc_scale.
    Each operand is None, a [n, d] tensor or a (lo, hi) pair of row blocks. vals: other
    values for the plan's pattern ([nnz] float32 in the plan's entry order; default
    plan.vals)."""
    from recbole_amd._native import SpmmEpilogue
    if vals is None:
        vals = plan.vals
    else:
        _dev(vals, torch.float32, "vals")
        if vals.shape != plan.vals.shape:
            raise ValueError(f"spmm_csr: vals shape {tuple(vals.shape)} != "
                             f"{tuple(plan.vals.shape)}")
    n, d = _rows_n(x)
    if n != plan.n_rows:
        raise ValueError(f"spmm_csr: x has {n} rows, the matrix {plan.n_rows}")
    for name, t in (("y", y), ("add", add), ("acc_in", acc_in), ("acc_out", acc_out)):
        if t is not None and _rows_n(t) != (n, d):
            raise ValueError(f"spmm_csr: {name} shape {_rows_n(t)} != {(n, d)}")
    if y is None and acc_out is None:
        raise ValueError("spmm_csr: nothing to write")
    dev = plan.row_ptr.device
    part = plan.partial(d, dev)
    ep = SpmmEpilogue(_rows_ref(add), add_scale, _rows_ref(y), _rows_ref(acc_in),
                      _rows_ref(acc_out), acc_scale)
    xr = _rows_ref(x)
    rc = lib().mirec_spmm_csr_f32(ptr(plan.row_ptr), ptr(plan.cols), ptr(vals), plan.n_rows,
                                  d, ptr(plan.unit_row), ptr(plan.unit_beg), ptr(plan.unit_slot),
                                  plan.n_units, plan.piece, ptr(plan.fix_row), ptr(plan.fix_ptr),
                                  plan.n_fix, ptr(part), ctypes.byref(xr), ctypes.byref(ep),
                                  stream_handle())
    check(rc, "mirec_spmm_csr_f32")


def gather_sqnorm(table, idx, out=None):
    """out[i] = ||table[idx[i]]||^2 (EmbLoss, loss.py:79-84)."""
    _dev(table, torch.float32, "table")
    _dev(idx, torch.int64, "idx")
    if out is None:
        out = torch.empty(idx.numel(), dtype=torch.float32, device=table.device)
    rc = lib().mirec_gather_sqnorm_f32(ptr(table), table.shape[0], table.shape[1], ptr(idx),
                                       idx.numel(), ptr(out), stream_handle())
    check(rc, "mirec_gather_sqnorm_f32")
    return out


def gather_scale_rows(table, idx, scale_dev, out=None):
    """out[i, :] = scale_dev[0] * table[idx[i], :]."""
    _dev(table, torch.float32, "table")
    _dev(idx, torch.int64, "idx")
    _dev(scale_dev, torch.float32, "scale")
    if out is None:
        out = torch.empty(idx.numel(), table.shape[1], dtype=torch.float32, device=table.device)
    rc = lib().mirec_gather_scale_rows_f32(ptr(table), table.shape[0], table.shape[1], ptr(idx),
                                           idx.numel(), ptr(scale_dev), ptr(out),
                                           stream_handle())
    check(rc, "mirec_gather_scale_rows_f32")
    return out


# ---------------------------------------------------------------- K16 NGCF bi-interaction
def _rows_ld(t, d: int, name: str):
    """(mirec_rows_ld, n rows) from None, a [n, d] float32 GPU tensor whose rows are
    contiguous (a column slice of a wider row-major buffer is fine) or a (lo, hi) pair of
    such blocks with one row stride."""
    from recbole_amd._native import RowsLd
    if t is None:
        return RowsLd(None, None, 0, 0), 0
    parts = t if isinstance(t, tuple) else (t,)
    for p in parts:
        if not isinstance(p, torch.Tensor):
            raise TypeError(f"{name} must be a torch.Tensor or a pair of them")
        if not p.is_cuda:
            raise NativeError(f"{name} must live on the GPU (got {p.device}); no CPU fallback "
                              f"exists")
        if p.dtype != torch.float32 or p.dim() != 2 or p.shape[1] != d:
            raise ValueError(f"{name} must be float32 [n, {d}], got {p.dtype} {tuple(p.shape)}")
        if p.stride(1) != 1 or p.stride(0) < d or p.stride(0) % 4 or p.data_ptr() % 16:
            raise ValueError(f"{name}: rows must be contiguous, 16-byte aligned, with a row "
                             f"stride that is a multiple of 4")
    if len(parts) == 2:
        lo, hi = parts
        if lo.stride(0) != hi.stride(0):
            raise ValueError(f"{name}: the two row blocks have different row strides")
        return RowsLd(ptr(lo), ptr(hi), lo.shape[0], lo.stride(0)), lo.shape[0] + hi.shape[0]
    return RowsLd(ptr(t), None, t.shape[0], t.stride(0)), t.shape[0]


def _drop_args(p, rng, drawn):
    """(seed, counter, drawn) of a dropout site as the kernels take them: p > 0 needs rng =
    (seed, device int64 counter) and the device int64 word `drawn`; p == 0 passes no words."""
    if not p:
        return 0, None, None
    seed, counter = rng
    _dev(counter, torch.int64, "counter")
    _dev(drawn, torch.int64, "drawn")
    return seed, counter, drawn


def ngcf_shape_ok(d_in: int, d_out: int) -> bool:
    """Whether K16 is built for a layer d_in -> d_out ({64, 128}^2)."""
    return lib().mirec_ngcf_shape_ok(int(d_in), int(d_out)) != 0


def ngcf_grid_cap(workgroups: int) -> int:
    """Cap the workgroups of K16a / K16b at `workgroups` (0: the chip decides; negative: only
    ask); returns the cap before the call. No output bit depends on it: the tests use it to
    make every wave walk many slabs at a small N."""
    return int(lib().mirec_ngcf_grid_cap(int(workgroups)))


def _ngcf_widths(what, W1, W2, b1=None, b2=None):
    _dev(W1, torch.float32, "W1")
    _dev(W2, torch.float32, "W2")
    d_out, d_in = W1.shape
    if W2.shape != W1.shape:
        raise ValueError(f"{what}: W1 {tuple(W1.shape)} and W2 {tuple(W2.shape)} differ")
    if not ngcf_shape_ok(d_in, d_out):
        raise NativeError(f"{what}: widths {d_in} -> {d_out} not in the built set ({{64,128}}^2)")
    for n_, b in (("b1", b1), ("b2", b2)):
        if b is not None:
            _dev(b, torch.float32, n_)
            if b.shape != (d_out,):
                raise ValueError(f"{what}: {n_} shape {tuple(b.shape)} != ({d_out},)")
    return d_in, d_out


def ngcf_layer_fwd(E, x, W1, b1, W2, b2, out, copy=None, p: float = 0.0, rng=None, drawn=None):
    """K16a: out = normalize(dropout_p(leaky_relu_0.2((E + x) W1^T + b1 + (x * E) W2^T + b2)))
    per row, written into `out` (a rows operand: typically a column slice of the [N, D]
    concat buffer) and optionally `copy` (contiguous [N, d_out]); returns nrm [N] = the row
    norms before the scale. E: a rows operand ([N, d_in] or the (user, item) table pair).
    p > 0: rng = (seed, device int64 counter), drawn = a device int64 word that takes the
    counter value used (the counter is advanced by the backward)."""
    d_in, d_out = _ngcf_widths("ngcf_layer_fwd", W1, W2, b1, b2)
    _dev(x, torch.float32, "x")
    Er, n = _rows_ld(E, d_in, "E")
    Or, n_o = _rows_ld(out, d_out, "out")
    if x.shape != (n, d_in) or n_o != n:
        raise ValueError(f"ngcf_layer_fwd: E has {n} rows, x {tuple(x.shape)}, out {n_o} rows")
    if copy is not None:
        _dev(copy, torch.float32, "copy")
        if copy.shape != (n, d_out):
            raise ValueError(f"ngcf_layer_fwd: copy shape {tuple(copy.shape)} != {(n, d_out)}")
    nrm = torch.empty(n, dtype=torch.float32, device=x.device)
    seed, counter, drawn = _drop_args(p, rng, drawn)
    rc = lib().mirec_ngcf_layer_fwd_f32(ctypes.byref(Er), ptr(x), n, d_in, d_out, ptr(W1), ptr(b1),
                                        ptr(W2), ptr(b2), ctypes.byref(Or), ptr(copy), ptr(nrm),
                                        float(p), seed, ptr(counter), ptr(drawn), stream_handle())
    check(rc, "mirec_ngcf_layer_fwd_f32")
    return nrm


def ngcf_layer_bwd(G, E_next, nrm, W1, W2, E, x, add=None, p: float = 0.0, rng=None, drawn=None):
    """K16b: from G (the gradient of a layer's output E_next, both rows operands) returns
    (gz [N, d_out], dE [N, d_in] = g_z W1 + (g_z W2) * x (+ add), gx [N, d_in] =
    g_z W1 + (g_z W2) * E); the layer's input gradient is A'^T gx + dE. p > 0 redraws the
    forward's keep bits from `drawn` and sets the counter of rng to drawn + 1."""
    d_in, d_out = _ngcf_widths("ngcf_layer_bwd", W1, W2)
    _dev(x, torch.float32, "x")
    _dev(nrm, torch.float32, "nrm")
    Gr, n = _rows_ld(G, d_out, "G")
    Nr, n_n = _rows_ld(E_next, d_out, "E_next")
    Er, n_e = _rows_ld(E, d_in, "E")
    Ar, n_a = _rows_ld(add, d_in, "add")
    if not (n_n == n_e == n) or x.shape != (n, d_in) or nrm.shape != (n,) or \
            (add is not None and n_a != n):
        raise ValueError("ngcf_layer_bwd: operands disagree on the number of rows")
    dev = x.device
    gz = torch.empty(n, d_out, dtype=torch.float32, device=dev)
    dE = torch.empty(n, d_in, dtype=torch.float32, device=dev)
    gx = torch.empty(n, d_in, dtype=torch.float32, device=dev)
    seed, counter, drawn = _drop_args(p, rng, drawn)
    rc = lib().mirec_ngcf_layer_bwd_f32(ctypes.byref(Gr), ctypes.byref(Nr), ptr(nrm), n, d_in,
                                        d_out, ptr(W1), ptr(W2), ctypes.byref(Er), ptr(x),
                                        ctypes.byref(Ar), ptr(gz), ptr(dE), ptr(gx), float(p),
                                        seed, ptr(drawn), ptr(counter), stream_handle())
    check(rc, "mirec_ngcf_layer_bwd_f32")
    return gz, dE, gx


def ngcf_wgrad(gz, E, x, d_in: int):
    """K16c + the finish: (dW1, dW2 [d_out, d_in], db [d_out]) = g_z^T (E + x), g_z^T (x * E)
    and the column sum of g_z, over the node rows in a fixed order."""
    _dev(gz, torch.float32, "gz")
    _dev(x, torch.float32, "x")
    n, d_out = gz.shape
    if not ngcf_shape_ok(d_in, d_out):
        raise NativeError(f"ngcf_wgrad: widths {d_in} -> {d_out} not in the built set "
                          f"({{64,128}}^2)")
    Er, n_e = _rows_ld(E, d_in, "E")
    if n_e != n or x.shape != (n, d_in) or n == 0:
        raise ValueError("ngcf_wgrad: operands disagree on the number of rows")
    dev = gz.device
    C = lib().mirec_ngcf_wgrad_splits(n)
    P = torch.empty(C, d_out, 2 * d_in, dtype=torch.float32, device=dev)
    check(lib().mirec_ngcf_wgrad_f32(ptr(gz), ctypes.byref(Er), ptr(x), n, d_in, d_out, ptr(P),
                                     stream_handle()), "mirec_ngcf_wgrad_f32")
    dW, db = linear_grad_finish(P, gz)
    return dW[:, :d_in].contiguous(), dW[:, d_in:].contiguous(), db


# ---------------------------------------------------------------- K18 xDeepFM CIN
def cin_shape_ok(m: int, H: int, D: int, N: int) -> bool:
    """Whether K18 is built for a layer of N channels over X0 [B, m, D], Xk [B, H, D]
    (m 2..64, H 1..256, D 1..64, N 2..256)."""
    return lib().mirec_cin_shape_ok(int(m), int(H), int(D), int(N)) != 0


def cin_grid_cap(workgroups: int) -> int:
    """Cap the workgroups of K18a / K18b at `workgroups` (0: the chip decides; negative: only
    ask); returns the cap before the call. No output bit depends on it."""
    return int(lib().mirec_cin_grid_cap(int(workgroups)))


def _cin_operands(what, X0, Xk, N, n_hid, dir0, W=None, b=None):
    _dev(X0, torch.float32, "X0")
    _dev(Xk, torch.float32, "Xk")
    if X0.dim() != 3 or Xk.dim() != 3 or Xk.shape[0] != X0.shape[0] or Xk.shape[2] != X0.shape[2]:
        raise ValueError(f"{what}: X0 {tuple(X0.shape)} and Xk {tuple(Xk.shape)} must be "
                         f"[B, m, D] and [B, H, D]")
    B, m, D = X0.shape
    H = Xk.shape[1]
    if not cin_shape_ok(m, H, D, N):
        raise NativeError(f"{what}: shape m {m}, H {H}, D {D}, N {N} not in the built set "
                          f"(m 2..64, H 1..256, D 1..64, N 2..256)")
    if not (0 <= n_hid <= N and 0 <= dir0 <= N):
        raise ValueError(f"{what}: channel split ({n_hid}, {dir0}) outside [0, {N}]")
    if W is not None:
        _dev(W, torch.float32, "W")
        if W.shape != (N, H * m):
            raise ValueError(f"{what}: W shape {tuple(W.shape)} != {(N, H * m)}")
    if b is not None:
        _dev(b, torch.float32, "b")
        if b.shape != (N,):
            raise ValueError(f"{what}: b shape {tuple(b.shape)} != ({N},)")
    return B, m, H, D


def _cin_pooled(what, t, name, B, N, dir0, pool_off):
    _dev(t, torch.float32, name)
    if t.dim() != 2 or t.shape[0] != B or pool_off < 0 or pool_off + (N - dir0) > t.shape[1]:
        raise ValueError(f"{what}: {name} {tuple(t.shape)} does not hold columns "
                         f"[{pool_off}, {pool_off + N - dir0}) of {B} rows")
    return t.shape[1]


def cin_layer_fwd(X0, Xk, W, b, n_hid: int, dir0: int, pooled, pool_off: int):
    """K18a: one CIN layer, out = b + W (Xk x X0) per (sample, dimension) row, never stored:
    returns X_{k+1} = out[:, :n_hid] as [B, n_hid, D] (None when n_hid == 0) and writes
    sum_d out[:, dir0:] into pooled[:, pool_off : pool_off + N - dir0]."""
    N = W.shape[0] if isinstance(W, torch.Tensor) else 0
    B, m, H, D = _cin_operands("cin_layer_fwd", X0, Xk, N, n_hid, dir0, W, b)
    ld = _cin_pooled("cin_layer_fwd", pooled, "pooled", B, N, dir0, pool_off)
    Xn = torch.empty(B, n_hid, D, dtype=torch.float32, device=X0.device) if n_hid else None
    with timed_launch('cin_fwd'):
        rc = lib().mirec_cin_layer_fwd_f32(ptr(X0), ptr(Xk), B, m, H, D, ptr(W), ptr(b), N, n_hid,
                                           dir0, ptr(Xn), ptr(pooled), pool_off, ld,
                                           stream_handle())
    check(rc, "mirec_cin_layer_fwd_f32")
    return Xn


def cin_layer_bwd(X0, Xk, W, n_hid: int, dir0: int, dXn, g_pooled, pool_off: int, dX0,
                  accumulate: bool, layer0: bool):
    """K18b: the data gradients of one CIN layer from dXn [B, n_hid, D] (or None) and the
    layer's columns of g_pooled. Returns dXk [B, H, D] (None for layer 0, whose Xk is X0) and
    writes (accumulate: adds) the X0 term — for layer 0 both terms — into dX0."""
    N = W.shape[0] if isinstance(W, torch.Tensor) else 0
    B, m, H, D = _cin_operands("cin_layer_bwd", X0, Xk, N, n_hid, dir0, W)
    ld = _cin_pooled("cin_layer_bwd", g_pooled, "g_pooled", B, N, dir0, pool_off)
    _dev(dX0, torch.float32, "dX0")
    if dX0.shape != X0.shape:
        raise ValueError(f"cin_layer_bwd: dX0 shape {tuple(dX0.shape)} != {tuple(X0.shape)}")
    if dXn is not None:
        _dev(dXn, torch.float32, "dXn")
        if dXn.shape != (B, n_hid, D):
            raise ValueError(f"cin_layer_bwd: dXn shape {tuple(dXn.shape)} != {(B, n_hid, D)}")
    if layer0 and (Xk.data_ptr() != X0.data_ptr() or H != m):
        raise ValueError("cin_layer_bwd: layer 0 takes Xk = X0")
    dXk = None if layer0 else torch.empty_like(Xk)
    with timed_launch('cin_bwd'):
        rc = lib().mirec_cin_layer_bwd_f32(ptr(X0), ptr(Xk), B, m, H, D, ptr(W), N, n_hid, dir0,
                                           ptr(dXn), ptr(g_pooled), pool_off, ld, ptr(dXk),
                                           ptr(dX0), 1 if accumulate else 0, stream_handle())
    check(rc, "mirec_cin_layer_bwd_f32")
    return dXk


def cin_wgrad(X0, Xk, N: int, n_hid: int, dir0: int, dXn, g_pooled, pool_off: int):
    """K18c + the finish: (dW [N, H m], db [N]) of one CIN layer, over the B D rows in a fixed
    order (per-split partials added in split order)."""
    B, m, H, D = _cin_operands("cin_wgrad", X0, Xk, N, n_hid, dir0)
    ld = _cin_pooled("cin_wgrad", g_pooled, "g_pooled", B, N, dir0, pool_off)
    if dXn is not None:
        _dev(dXn, torch.float32, "dXn")
        if dXn.shape != (B, n_hid, D):
            raise ValueError(f"cin_wgrad: dXn shape {tuple(dXn.shape)} != {(B, n_hid, D)}")
    if B == 0:
        raise ValueError("cin_wgrad: no rows")
    dev = X0.device
    K = H * m
    C = lib().mirec_cin_wgrad_splits(B, m, H, D)
    stride = lib().mirec_cin_wgrad_stride(N, K)
    P = torch.empty(C, stride, dtype=torch.float32, device=dev)
    with timed_launch('cin_wgrad'):
        rc = lib().mirec_cin_wgrad_f32(ptr(X0), ptr(Xk), B, m, H, D, N, n_hid, dir0, ptr(dXn),
                                       ptr(g_pooled), pool_off, ld, ptr(P), stream_handle())
    check(rc, "mirec_cin_wgrad_f32")
    out, _ = linear_grad_finish(P)
    nw = (N * K + 3) // 4 * 4
    return out[:N * K].view(N, K), out[nw:nw + N]


# ---------------------------------------------------------------- K19 DCN cross network
def cross_shape_ok(n: int, L: int) -> bool:
    """Whether K19 is built for L cross layers over rows of n floats (n 2..1024, L 1..8)."""
    return lib().mirec_cross_shape_ok(int(n), int(L)) != 0


def cross_grid_cap(workgroups: int) -> int:
    """Cap the workgroups of K19a / K19b at `workgroups` (0: the chip decides; negative: only
    ask); returns the cap before the call. No output bit depends on it."""
    return int(lib().mirec_cross_grid_cap(int(workgroups)))


def _cross_operands(what, x0, W, Bv, wp=None):
    _dev(x0, torch.float32, "x0")
    _dev(W, torch.float32, "W")
    _dev(Bv, torch.float32, "Bv")
    if x0.dim() != 2 or W.dim() != 2 or W.shape[1] != x0.shape[1] or Bv.shape != W.shape:
        raise ValueError(f"{what}: x0 {tuple(x0.shape)}, W {tuple(W.shape)} and Bv "
                         f"{tuple(Bv.shape)} must be [B, n], [L, n] and [L, n]")
    B, n = x0.shape
    L = W.shape[0]
    if not cross_shape_ok(n, L):
        raise NativeError(f"{what}: shape n {n}, L {L} not in the built set (n 2..1024, L 1..8)")
    if wp is not None:
        _dev(wp, torch.float32, "wp")
        if wp.shape != (n,):
            raise ValueError(f"{what}: wp shape {tuple(wp.shape)} != ({n},)")
    return B, n, L


def cross_fwd(x0, W, Bv, wp=None, want_xL=None):
    """K19a: the cross network x_{l+1} = x0 (x_l . w_l) + b_l + x_l over x0 [B, n] with W, Bv
    [L, n], no x_l stored. Returns (S [B, L] with s_l = x_l . w_l, y [B] = x_L . wp or None
    without wp, x_L [B, n] or None). want_xL defaults to `wp is None` (plain mode)."""
    B, n, L = _cross_operands("cross_fwd", x0, W, Bv, wp)
    if want_xL is None:
        want_xL = wp is None
    if wp is None and not want_xL:
        raise ValueError("cross_fwd: nothing asked for (neither wp nor x_L)")
    dev = x0.device
    S = torch.empty(B, L, dtype=torch.float32, device=dev)
    y = torch.empty(B, dtype=torch.float32, device=dev) if wp is not None else None
    xL = torch.empty(B, n, dtype=torch.float32, device=dev) if want_xL else None
    with timed_launch('cross_fwd'):
        rc = lib().mirec_cross_fwd_f32(ptr(x0), B, n, ptr(W), ptr(Bv), L, ptr(wp), ptr(S), ptr(y),
                                       ptr(xL), stream_handle())
    check(rc, "mirec_cross_fwd_f32")
    return S, y, xL


def cross_bwd(x0, W, Bv, S, wp=None, gy=None, gL=None):
    """K19b + the finish: the gradients of the cross network for g_L = gy wp + gL (head mode:
    wp and gy [B] together; plain mode: gL [B, n]; at least one). Returns (dx0 [B, n],
    dW [L, n], dB [L, n], dwp [n] — zero without head mode), the three weight parts being
    views of one finished [2L + 1, n] block summed over the rows in a fixed order."""
    B, n, L = _cross_operands("cross_bwd", x0, W, Bv, wp)
    _dev(S, torch.float32, "S")
    if S.shape != (B, L):
        raise ValueError(f"cross_bwd: S shape {tuple(S.shape)} != {(B, L)}")
    if (wp is None) != (gy is None):
        raise ValueError("cross_bwd: wp and gy come together (head mode)")
    if gy is None and gL is None:
        raise ValueError("cross_bwd: neither gy nor gL given")
    if gy is not None:
        _dev(gy, torch.float32, "gy")
        if gy.shape != (B,):
            raise ValueError(f"cross_bwd: gy shape {tuple(gy.shape)} != ({B},)")
    if gL is not None:
        _dev(gL, torch.float32, "gL")
        if gL.shape != (B, n):
            raise ValueError(f"cross_bwd: gL shape {tuple(gL.shape)} != {(B, n)}")
    if B == 0:
        raise ValueError("cross_bwd: no rows")
    dev = x0.device
    C = lib().mirec_cross_bwd_splits(B, n, L)
    stride = lib().mirec_cross_bwd_stride(n, L)
    P = torch.empty(C, stride, dtype=torch.float32, device=dev)
    dx0 = torch.empty_like(x0)
    with timed_launch('cross_bwd'):
        rc = lib().mirec_cross_bwd_f32(ptr(x0), B, n, ptr(W), ptr(Bv), L, ptr(S), ptr(wp), ptr(gy),
                                       ptr(gL), ptr(dx0), ptr(P), stream_handle())
    check(rc, "mirec_cross_bwd_f32")
    out, _ = linear_grad_finish(P)
    block = out[:(2 * L + 1) * n].view(2 * L + 1, n)
    return dx0, block[:L], block[L:2 * L], block[2 * L]


# ---------------------------------------------------------------- K20 AFM pairwise attention
def afm_shape_ok(F: int, d: int, A: int) -> bool:
    """Whether K20 is built for F fields of width d and attention size A (F 2..64, d 2..64,
    A 1..64)."""
    return lib().mirec_afm_shape_ok(int(F), int(d), int(A)) != 0


def afm_grid_cap(workgroups: int) -> int:
    """Cap the workgroups of K20a / K20b at `workgroups` (0: the chip decides; negative: only
    ask); returns the cap before the call. No output bit depends on it."""
    return int(lib().mirec_afm_grid_cap(int(workgroups)))


def _afm_operands(what, X, W, h, pv):
    _dev(X, torch.float32, "X")
    _dev(W, torch.float32, "W")
    _dev(h, torch.float32, "h")
    _dev(pv, torch.float32, "pv")
    if X.dim() != 3 or W.dim() != 2 or W.shape[1] != X.shape[2] or h.shape != (W.shape[0],) or \
            pv.shape != (X.shape[2],):
        raise ValueError(f"{what}: X {tuple(X.shape)}, W {tuple(W.shape)}, h {tuple(h.shape)} and "
                         f"pv {tuple(pv.shape)} must be [B, F, d], [A, d], [A] and [d]")
    B, F, d = X.shape
    A = W.shape[0]
    if not afm_shape_ok(F, d, A):
        raise NativeError(f"{what}: shape F {F}, d {d}, A {A} not in the built set (F 2..64, "
                          f"d 2..64, A 1..64)")
    return B, F, d, A


def afm_fwd(X, W, h, pv, p: float = 0.0, rng=None, drawn=None):
    """K20a: y [B] = dropout_p(sum_p alpha_p (e_i * e_j)) . pv with alpha the softmax over the
    pairs of h . relu(W (e_i * e_j)), from the field rows X [B, F, d]; no pair tensor is
    stored. Returns (y, V [B, d] — the pooled vector before dropout, ML [B, 2] — the softmax
    maximum and sum). p > 0: rng = (seed, device int64 counter), drawn = a device int64 word
    that takes the counter value used (the counter is advanced by the backward)."""
    B, F, d, A = _afm_operands("afm_fwd", X, W, h, pv)
    dev = X.device
    y = torch.empty(B, dtype=torch.float32, device=dev)
    V = torch.empty(B, d, dtype=torch.float32, device=dev)
    ML = torch.empty(B, 2, dtype=torch.float32, device=dev)
    seed, counter, drawn = _drop_args(p, rng, drawn)
    with timed_launch('afm_fwd'):
        rc = lib().mirec_afm_fwd_f32(ptr(X), B, F, d, ptr(W), ptr(h), A, ptr(pv), ptr(y), ptr(V),
                                     ptr(ML), float(p), seed, ptr(counter), ptr(drawn),
                                     stream_handle())
    check(rc, "mirec_afm_fwd_f32")
    return y, V, ML


def afm_bwd(X, W, h, pv, V, ML, gy, p: float = 0.0, rng=None, drawn=None):
    """K20b + the finish: (dX [B, F, d], dW [A, d], dh [A], dpv [d]) for the upstream gy [B],
    the three weight parts being views of one finished block summed over the rows in a fixed
    order. p > 0 redraws the forward's keep flags from `drawn` and sets the counter of rng to
    drawn + 1."""
    B, F, d, A = _afm_operands("afm_bwd", X, W, h, pv)
    _dev(V, torch.float32, "V")
    _dev(ML, torch.float32, "ML")
    _dev(gy, torch.float32, "gy")
    if V.shape != (B, d) or ML.shape != (B, 2) or gy.shape != (B,):
        raise ValueError(f"afm_bwd: V {tuple(V.shape)}, ML {tuple(ML.shape)} and gy "
                         f"{tuple(gy.shape)} must be {(B, d)}, {(B, 2)} and ({B},)")
    if B == 0:
        raise ValueError("afm_bwd: no rows")
    dev = X.device
    C = lib().mirec_afm_bwd_splits(B, F, d, A)
    stride = lib().mirec_afm_bwd_stride(d, A)
    P = torch.empty(C, stride, dtype=torch.float32, device=dev)
    dX = torch.empty_like(X)
    seed, counter, drawn = _drop_args(p, rng, drawn)
    with timed_launch('afm_bwd'):
        rc = lib().mirec_afm_bwd_f32(ptr(X), B, F, d, ptr(W), ptr(h), A, ptr(pv), ptr(V), ptr(ML),
                                     ptr(gy), ptr(dX), ptr(P), float(p), seed, ptr(drawn),
                                     ptr(counter), stream_handle())
    check(rc, "mirec_afm_bwd_f32")
    out, _ = linear_grad_finish(P)
    return dX, out[:A * d].view(A, d), out[A * d:A * d + A], out[A * d + A:A * d + A + d]
