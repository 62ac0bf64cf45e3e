"""Thin torch-tensor wrappers over the C ABI (one function per entry point).

Every wrapper checks device / dtype / contiguity, allocates outputs with torch (the
library never allocates) and enqueues on torch's current stream.  No arithmetic
happens here: if the HIP extension is missing these raise `HipExtensionError`.
"""
from __future__ import annotations

from typing import Optional

import ctypes
import math
import numbers

import numpy as np
import torch

from . import constants as C
from ._lib import PLAN_FIELDS, HipExtensionError, call, lib, plan_layout, ptr, stream

F32, I32, I64, U8, F64 = torch.float32, torch.int32, torch.int64, torch.uint8, torch.float64

# Optional per-launch timing with HIP events on the launch stream (used by bench.py for the roofline
# figures): PROF = {"kernel class": [(start_event, end_event, algorithmic_work), ...]} or None.
PROF = None


def _prof_begin(name: str):
    if PROF is None:
        return None
    PROF.setdefault(name, [])
    e0 = torch.cuda.Event(enable_timing=True)
    e0.record()
    return e0


def _prof_end(name: str, e0, work: float):
    if e0 is not None:
        e1 = torch.cuda.Event(enable_timing=True)
        e1.record()
        PROF[name].append((e0, e1, work))


_GEMM_TILES = ("64x64x16", "128x128x16", "64x64x32", "128x128x32", "x6:128x128x16", "x6:128x64x16", "x6:64x64x32",
               "x6:128x128x32", "planes:64x64x32", "planesB:64x128x32", "planes:128x128x32")
# Tile names by configuration id (the profiler's class numbering follows the same ids).  The library builds and launches
# only the live ids; 1, 3, 6 and 10 are retired and keep their place in the list.  pm_gemm_force_config pins an fp32 or
# x6 id; the planes configurations follow from the operands of a call.
GEMM_LIVE_IDS = (0, 2, 4, 5, 7, 8, 9)
GEMM_PIN_IDS = (0, 2, 4, 5, 7)


def gemm_class(transA: bool, transB: bool, M: int, N: int, K: int) -> str:
    """Kernel instance a plain GEMM call maps to: the library's own choice for one group, no row map and 16-byte
    aligned fp32 operands (pm_gemm_config), which is what the launch runs for such a call."""
    from ._lib import lib
    return f"gemm_{'T' if transA else 'N'}{'T' if transB else 'N'}_{_GEMM_TILES[lib().pm_gemm_config(int(transA), M, N, K)]}"


def _chk(t: Optional[torch.Tensor], dtype, name: str, allow_none=False):
    if t is None:
        if allow_none:
            return
        raise ValueError(f"{name} is None")
    if not t.is_cuda:
        raise HipExtensionError(f"{name} lives on {t.device}: the HIP path needs device tensors (no CPU fallback)")
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")


class Plan:
    """Device-side graph plan of one batch (see include/polyphemus_hip.h, pm_plan_build)."""

    def __init__(self, buf: torch.Tensor, N: int, E: int, G: int, n_bars: int, tokens: torch.Tensor,
                 is_drum: torch.Tensor):
        self.buf, self.N, self.E, self.G, self.n_bars = buf, N, E, G, n_bars
        self.B = G // n_bars
        self.tokens, self.is_drum = tokens, is_drum
        self._off = plan_layout(N, E, G)

    def field(self, name: str) -> torch.Tensor:
        i = PLAN_FIELDS.index(name)
        v = self.buf[self._off[i]:self._off[i + 1]]
        return v.view(torch.float32) if name == "csc_invcnt" else v

    @property
    def tok_hist(self) -> torch.Tensor:
        return self.field("tok_hist")

    @property
    def drum_list(self) -> torch.Tensor:
        return self.field("group_list")[:self.N]

    @property
    def nondrum_list(self) -> torch.Tensor:
        return self.field("group_list")[self.N:2 * self.N]

    @property
    def drum_rows(self) -> torch.Tensor:
        """(node, slot) rows node*15+slot of the drum nodes (first 15*n_drum entries are live)."""
        return self.field("row_list")[:self.N * C.N_SLOTS]

    @property
    def nondrum_rows(self) -> torch.Tensor:
        return self.field("row_list")[self.N * C.N_SLOTS:2 * self.N * C.N_SLOTS]

    @property
    def group_cnt(self) -> torch.Tensor:
        """[n_drum, n_non_drum, 15*n_drum, 15*n_non_drum] (device)."""
        return self.field("group_cnt")


def edge_attrs_to_ids(edge_attrs: torch.Tensor):
    _chk(edge_attrs, F32, "edge_attrs")
    E = edge_attrs.shape[0]
    et = torch.empty(E, dtype=I32, device=edge_attrs.device)
    ed = torch.empty(E, dtype=I32, device=edge_attrs.device)
    call("pm_edge_attrs_to_ids", ptr(edge_attrs), E, ptr(et), ptr(ed), stream())
    return et, ed


def tokens_from_onehot(c_tensor: torch.Tensor) -> torch.Tensor:
    _chk(c_tensor, F32, "c_tensor")
    N = c_tensor.shape[0]
    tok = torch.empty(N, 16, 2, dtype=I32, device=c_tensor.device)
    call("pm_tokens_from_onehot", ptr(c_tensor), N, ptr(tok), stream())
    return tok


def plan_build(edge_index, edge_type, edge_dist, bars, batch, is_drum, tokens, n_bars: int, G: int,
               n_slots: int = C.N_SLOTS) -> Plan:
    _chk(edge_index, I64, "edge_index"); _chk(edge_type, I32, "edge_type"); _chk(edge_dist, I32, "edge_dist")
    _chk(bars, I64, "bars"); _chk(batch, I64, "batch"); _chk(tokens, I32, "tokens")
    if is_drum.dtype == torch.bool:
        is_drum = is_drum.view(U8)
    _chk(is_drum, U8, "is_drum")
    N, E = bars.shape[0], edge_index.shape[1]
    off = plan_layout(N, E, G)
    buf = torch.empty(off[-1], dtype=I32, device=bars.device)
    call("pm_plan_build", ptr(edge_index), ptr(edge_type), ptr(edge_dist), ptr(bars), ptr(batch), ptr(is_drum),
         ptr(tokens), n_bars, n_slots, N, E, G, ptr(buf), stream())
    return Plan(buf, N, E, G, n_bars, tokens, is_drum)


def edge_table(nn_weight, nn_bias):
    _chk(nn_weight, F32, "nn.weight"); _chk(nn_bias, F32, "nn.bias")
    d = nn_weight.shape[0]
    T = torch.empty(C.N_DISTS, d, dtype=F32, device=nn_weight.device)
    call("pm_edge_table", ptr(nn_weight), ptr(nn_bias), d, ptr(T), stream())
    return T


def edge_table_bwd(dT, d_nn_weight, d_nn_bias):
    call("pm_edge_table_bwd", ptr(dT), dT.shape[1], ptr(d_nn_weight), ptr(d_nn_bias), stream())


def graph_build(s_tensor: torch.Tensor, n_bars: int, sizes=None):
    """Bar graphs of a batch on the device (`pm_graph_count` + `pm_graph_emit`): `s_tensor` float32 [G,4,32] 0/1
    (empty bars get cell [0,0] switched on in place, data.py:152-153).  Returns a dict of device tensors with the
    reference's node numbering and edge order; ONE host read (N, E) sizes the outputs.  A caller that knows the totals
    passes `sizes=(N, E)`: they are trusted, nothing is read back, and the device's own totals come along as `totals`
    (int32 [2]) for a later comparison (`ResidentDataset.batch`, whose counts are host arithmetic)."""
    if sizes is not None and not (isinstance(sizes, (tuple, list)) and len(sizes) == 2 and all(_integer(v) and 1 <= v < (1 << 31) for v in sizes)):
        raise ValueError(f"sizes must be None or two ints (N, E) in [1, 2^31), got {sizes!r}")
    _chk(s_tensor, F32, "s_tensor")
    G = s_tensor.shape[0]
    dev = s_tensor.device
    bn, be = torch.empty(G, dtype=I32, device=dev), torch.empty(G, dtype=I32, device=dev)
    npt, ept = torch.empty(G + 1, dtype=I32, device=dev), torch.empty(G + 1, dtype=I32, device=dev)
    tot = torch.empty(2, dtype=I32, device=dev)
    call("pm_graph_count", ptr(s_tensor), G, ptr(bn), ptr(be), ptr(npt), ptr(ept), ptr(tot), stream())
    if sizes is None:
        N, E = (int(v) for v in tot.tolist())
    else:
        N, E = int(sizes[0]), int(sizes[1])
    out = dict(edge_index=torch.empty(2, E, dtype=I64, device=dev), edge_type=torch.empty(E, dtype=I32, device=dev),
               edge_dist=torch.empty(E, dtype=I32, device=dev), bars=torch.empty(N, dtype=I64, device=dev),
               batch=torch.empty(N, dtype=I64, device=dev), is_drum=torch.empty(N, dtype=U8, device=dev),
               node_cell=torch.empty(N, dtype=I32, device=dev), node_ptr=npt, edge_ptr=ept, num_nodes=N)
    call("pm_graph_emit", ptr(s_tensor), G, n_bars, ptr(npt), ptr(ept), N, E, ptr(out["edge_index"]), ptr(out["edge_type"]),
         ptr(out["edge_dist"]), ptr(out["bars"]), ptr(out["batch"]), ptr(out["is_drum"]), ptr(out["node_cell"]), stream())
    out["is_drum"] = out["is_drum"].view(torch.bool)
    if sizes is not None:
        out["totals"] = tot
    return out


def _dataset_store_args(s_bits, rows, cell_ptr, n_bars):
    """The checks the readers of the resident store share: `s_bits` int32 [n,n_bars,4] (the bits of the ABI's uint32 words),
    `rows` uint8 [R,16,2], `cell_ptr` int64 [n+1] (ValueError); returns (n, R)."""
    for t, name in ((s_bits, "s_bits"), (rows, "rows"), (cell_ptr, "cell_ptr")):
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{name} must be a tensor, got {type(t).__name__}")
    if not (_integer(n_bars) and 1 <= n_bars <= MAX_DATASET_BARS):
        raise ValueError(f"n_bars must be an int in [1, {MAX_DATASET_BARS}], got {n_bars!r}")
    if s_bits.dtype != I32 or s_bits.dim() != 3 or s_bits.shape[0] < 1 or tuple(s_bits.shape[1:]) != (n_bars, 4):
        raise ValueError(f"s_bits must be int32 [n,{n_bars},4] with n >= 1, got {s_bits.dtype} {tuple(s_bits.shape)}")
    if rows.dtype != U8 or rows.dim() != 3 or rows.shape[0] < 1 or tuple(rows.shape[1:]) != (C.MAX_SIMU_TOKENS, 2):
        raise ValueError(f"rows must be uint8 [R,16,2] with R >= 1, got {rows.dtype} {tuple(rows.shape)}")
    n = s_bits.shape[0]
    if cell_ptr.dtype != I64 or tuple(cell_ptr.shape) != (n + 1,):
        raise ValueError(f"cell_ptr must be int64 [n + 1 = {n + 1}], got {cell_ptr.dtype} {tuple(cell_ptr.shape)}")
    return n, rows.shape[0]


MAX_DATASET_BARS = 64


def dataset_pack(token_grid: torch.Tensor, s_grid: torch.Tensor, rows: Optional[torch.Tensor] = None, row_base: int = 0):
    """`pm_dataset_pack_count` + `pm_dataset_pack_rows` ("Resident data set" in include/polyphemus_hip.h): a chunk of samples
    in `PolyphemusDataset`'s layout, `token_grid` int16 [n,n_bars,4,32,16,2] and `s_grid` uint8 [n,n_bars,4,32], packed into
    the compact store.  The chunk's rows go to `rows` (uint8 [capacity,16,2]) from row `row_base` on; a missing or too small
    buffer is replaced by a larger one that keeps the rows in front of `row_base`.  Returns a dict: s_bits int32 [n,n_bars,4],
    rows (the buffer written), cells / edges / last_slot (numpy int32 [n]: nodes, edges and last live token slot per sample;
    the edges are `pm_graph_count`'s on the chunk's structure) and total (the chunk's rows).  ONE host read per chunk brings
    the counts; token ids of active cells outside their ranges raise ValueError with their number.  Runs once per data set."""
    for t, name in ((token_grid, "token_grid"), (s_grid, "s_grid")):
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{name} must be a tensor, got {type(t).__name__}")
    if token_grid.dtype != torch.int16 or token_grid.dim() != 6 or token_grid.shape[0] < 1 or token_grid.shape[1] < 1 or \
            tuple(token_grid.shape[2:]) != (C.N_TRACKS, C.N_TIMESTEPS, C.MAX_SIMU_TOKENS, 2):
        raise ValueError(f"token_grid must be int16 [n,n_bars,4,32,16,2], got {token_grid.dtype} {tuple(token_grid.shape)}")
    n, n_bars = int(token_grid.shape[0]), int(token_grid.shape[1])
    if n_bars > MAX_DATASET_BARS:
        raise ValueError(f"token_grid: n_bars must be at most {MAX_DATASET_BARS}, got {n_bars}")
    if s_grid.dtype != U8 or tuple(s_grid.shape) != (n, n_bars, C.N_TRACKS, C.N_TIMESTEPS):
        raise ValueError(f"s_grid must be uint8 [{n},{n_bars},4,32], got {s_grid.dtype} {tuple(s_grid.shape)}")
    if 128 * n * n_bars > 0x7fffffff:
        raise ValueError(f"token_grid: a chunk holds at most 2^31 cells, got n = {n} samples of {n_bars} bars")
    if rows is not None and not (isinstance(rows, torch.Tensor) and rows.dtype == U8 and rows.dim() == 3
                                 and tuple(rows.shape[1:]) == (C.MAX_SIMU_TOKENS, 2)):
        raise ValueError("rows must be None or a uint8 tensor [capacity,16,2]")
    if not (_integer(row_base) and 0 <= row_base <= (0 if rows is None else rows.shape[0])):
        raise ValueError(f"row_base must be an int inside the rows buffer, got {row_base!r}")
    _on_device([(token_grid, "token_grid"), (s_grid, "s_grid")] + ([(rows, "rows")] if rows is not None else []))
    token_grid, s_grid, row_base, dev = token_grid.contiguous(), s_grid.contiguous(), int(row_base), token_grid.device
    s_bits = torch.empty(n, n_bars, 4, dtype=I32, device=dev)
    counts = torch.zeros(2 * n + 1, dtype=I32, device=dev)                         # cells, last_slot, status
    call("pm_dataset_pack_count", ptr(token_grid), ptr(s_grid), n, n_bars, ptr(s_bits), ptr(counts), ptr(counts[n:]),
         ptr(counts[2 * n:]), stream())
    G = n * n_bars
    s_f32 = s_grid.view(G, C.N_TRACKS, C.N_TIMESTEPS).to(F32)
    bn, be = torch.empty(G, dtype=I32, device=dev), torch.empty(G, dtype=I32, device=dev)
    scan = torch.empty(2 * G + 4, dtype=I32, device=dev)
    call("pm_graph_count", ptr(s_f32), G, ptr(bn), ptr(be), ptr(scan), ptr(scan[G + 1:]), ptr(scan[2 * G + 2:]), stream())
    host = torch.cat([counts, be.view(n, n_bars).sum(dim=1, dtype=I32)]).cpu().numpy()     # the one host read
    cells, last_slot, bad, edges = host[:n], host[n:2 * n], int(host[2 * n]), host[2 * n + 1:]
    if bad:
        raise ValueError(f"token_grid: {bad} token ids of active cells outside their ranges (pitch [0, {C.N_PITCH_TOKENS}), "
                         f"duration [0, {C.N_DUR_TOKENS}))")
    cell_off = np.zeros(n + 1, np.int64)
    np.cumsum(cells, out=cell_off[1:])
    total = int(cell_off[-1])
    if rows is None or rows.shape[0] < row_base + total:
        grown = torch.empty(max(row_base + total, 2 * (0 if rows is None else rows.shape[0])), C.MAX_SIMU_TOKENS, 2, dtype=U8, device=dev)
        if row_base:
            grown[:row_base] = rows[:row_base]
        rows = grown
    elif not rows.is_contiguous():
        raise ValueError("rows must be contiguous")
    cell_off_d = torch.from_numpy(cell_off).to(dev)
    call("pm_dataset_pack_rows", ptr(token_grid), ptr(s_bits), ptr(cell_off_d), n, n_bars, ptr(rows), row_base, rows.shape[0],
         stream())
    return dict(s_bits=s_bits, rows=rows, cells=cells.copy(), edges=edges.copy(), last_slot=last_slot.copy(), total=total)


def dataset_gather(s_bits: torch.Tensor, rows: torch.Tensor, cell_ptr: torch.Tensor, n_bars: int, index: torch.Tensor,
                   out_ptr: torch.Tensor, N: int, transpose: Optional[torch.Tensor] = None):
    """`pm_dataset_gather` ("Resident data set" in include/polyphemus_hip.h): the batch whose entry j is sample `index[j]` of
    the store (`s_bits` int32 [n,n_bars,4], `rows` uint8 [R,16,2], `cell_ptr` int64 [n+1]), in ONE launch.  `index` int32 [B]
    and `out_ptr` int32 [B+1] (the entries' row offsets, `N` = out_ptr[B] rows in all) are device tensors the caller computed
    on the host; `transpose` is None or int32 [B] semitones for the pitches of tracks 1..3.  Returns (s_tensor fp32
    [B n_bars,4,32], tokens int32 [N,16,2], status int32 [2] = indices outside [0, n), spans that do not match the store).
    An entry that is counted gets a structure of zeros and no rows; nothing is read back."""
    _dataset_store_args(s_bits, rows, cell_ptr, n_bars)
    if not isinstance(index, torch.Tensor) or index.dtype != I32 or index.dim() != 1 or index.shape[0] < 1:
        raise ValueError("index must be an int32 tensor [B] with B >= 1, got "
                         + (f"{index.dtype} {tuple(index.shape)}" if isinstance(index, torch.Tensor) else type(index).__name__))
    B = index.shape[0]
    if not isinstance(out_ptr, torch.Tensor) or out_ptr.dtype != I32 or tuple(out_ptr.shape) != (B + 1,):
        raise ValueError(f"out_ptr must be an int32 tensor [B + 1 = {B + 1}], got "
                         + (f"{out_ptr.dtype} {tuple(out_ptr.shape)}" if isinstance(out_ptr, torch.Tensor) else type(out_ptr).__name__))
    if transpose is not None and not (isinstance(transpose, torch.Tensor) and transpose.dtype == I32 and tuple(transpose.shape) == (B,)):
        raise ValueError(f"transpose must be None or an int32 tensor [B = {B}], got "
                         + (f"{transpose.dtype} {tuple(transpose.shape)}" if isinstance(transpose, torch.Tensor) else type(transpose).__name__))
    if not (_integer(N) and 1 <= N <= min(0x7fffffff, 128 * n_bars * B)):
        raise ValueError(f"N must be an int in [1, 128 n_bars B = {128 * n_bars * B}] below 2^31, got {N!r}")
    if 128 * n_bars * B > 0x7fffffff:
        raise ValueError(f"index: a batch holds at most 2^31 cells, got B = {B} entries of {n_bars} bars")
    named = [(s_bits, "s_bits"), (rows, "rows"), (cell_ptr, "cell_ptr"), (index, "index"), (out_ptr, "out_ptr")]
    _on_device(named + ([(transpose, "transpose")] if transpose is not None else []))
    for t, name in named + [(transpose, "transpose")]:
        if t is not None and not t.is_contiguous():
            raise ValueError(f"{name} must be contiguous")
    dev, N, n_bars = s_bits.device, int(N), int(n_bars)
    s = torch.empty(B * n_bars, C.N_TRACKS, C.N_TIMESTEPS, dtype=F32, device=dev)
    tokens = torch.empty(N, C.MAX_SIMU_TOKENS, 2, dtype=I32, device=dev)
    status = torch.zeros(2, dtype=I32, device=dev)
    call("pm_dataset_gather", ptr(s_bits), ptr(rows), ptr(cell_ptr), s_bits.shape[0], n_bars, rows.shape[0], ptr(index),
         ptr(out_ptr), ptr(transpose), B, N, ptr(s), ptr(tokens), ptr(status), stream())
    return s, tokens, status


def binary_from_logits(s_logits: torch.Tensor, thresh: float = 0.5) -> torch.Tensor:
    """`Decoder._binary_from_logits` (model.py:609-623) without the `nonzero` sync: bool tensor of s_logits' shape."""
    _chk(s_logits, F32, "s_logits")
    if s_logits.shape[-2:] != (4, 32):
        raise ValueError("s_logits must be [..., 4, 32]")
    out = torch.empty(s_logits.shape, dtype=U8, device=s_logits.device)
    call("pm_binary_from_logits", ptr(s_logits), s_logits.numel() // 128, float(thresh), None, ptr(out), stream())
    return out.view(torch.bool)


def _structure_prologue(s_tensor: torch.Tensor, dev, shape_ok: bool, message: str, segments: bool = False):
    """What the entry points that number the nodes of a structure share: the shape check (`shape_ok` and [...,4,32], else
    ValueError(message)), the structure as fp32 contiguous, its bar count G and the int32 scratch bar_nodes [G] and
    node_ptr [G+1] on `dev`; with `segments` also seg_count [4G] and seg_ptr [4G+1], the four cut from one allocation (a
    split costs about what an allocation does, so two pieces are two allocations).  Returns (s, G, *scratch)."""
    if not shape_ok or s_tensor.shape[-2:] != (4, 32):
        raise ValueError(message)
    s = s_tensor.to(F32).contiguous()
    G = s.numel() // 128
    if segments:
        return (s, G, *torch.empty(10 * G + 2, dtype=I32, device=dev).split([G, G + 1, 4 * G, 4 * G + 1]))
    return s, G, torch.empty(G, dtype=I32, device=dev), torch.empty(G + 1, dtype=I32, device=dev)


def _check_active(active: torch.Tensor, N: int, asked: str) -> None:
    """The node-count check of those entry points: reads the active-cell count back (the call's one host sync)."""
    active = int(active)
    if active != N:
        raise ValueError(f"shape mismatch: s_tensor has {active} active cells, {asked}")


def _mtp(entry: str, operand: torch.Tensor, name: str, s_tensor: torch.Tensor, check: bool) -> torch.Tensor:
    s, G, bn, npt = _structure_prologue(s_tensor, operand.device, s_tensor.dim() == 4, "s_tensor must be [B,n_bars,4,32]")
    N = operand.shape[0]
    mtp = torch.empty(*s_tensor.shape, C.MAX_SIMU_TOKENS - 1, C.D_TOKEN_PAIR, dtype=F32, device=operand.device)
    call(entry, ptr(operand), ptr(s), G, N, ptr(bn), ptr(npt), ptr(mtp), stream())
    if check:
        _check_active(npt[G], N, f"{name} has {N} nodes")
    return mtp


def mtp_from_logits(c_logits: torch.Tensor, s_tensor: torch.Tensor, check: bool = True) -> torch.Tensor:
    """`mtp_from_logits` (utils.py:59-79): [B,nb,4,32,15,230] with the nodes' logits on the active cells of `s_tensor`
    ([B,nb,4,32], any dtype) and hard silences elsewhere.  `check` reads the active-cell count back (one host sync) and
    raises like the reference's masked assignment when it differs from c_logits' node count."""
    _chk(c_logits, F32, "c_logits")
    if c_logits.dim() != 3 or c_logits.shape[1:] != (C.MAX_SIMU_TOKENS - 1, C.D_TOKEN_PAIR):
        raise ValueError("c_logits must be [N,15,230]")
    return _mtp("pm_mtp_from_logits", c_logits, "c_logits", s_tensor, check)


def _real(v) -> bool:
    return isinstance(v, numbers.Real) and not isinstance(v, bool)


def _integer(v) -> bool:
    return isinstance(v, numbers.Integral) and not isinstance(v, bool)


def _four(v, name: str):
    """An int or four ints (one per track) as a tuple of four ints."""
    out = tuple(v) if isinstance(v, (tuple, list, np.ndarray)) else (v,) * 4
    if len(out) != 4 or not all(_integer(a) for a in out):
        raise ValueError(f"{name} must be an int or four ints (one per track), got {v!r}")
    return tuple(int(a) for a in out)


def _mask_words(array, shape, name: str):
    """A bool array-like of `shape` = (4, 32 w) as 4 x w words of 32 bits (bit b of word j = element 32 j + b); None = all set."""
    if array is None:
        return [[0xFFFFFFFF] * (shape[1] // 32) for _ in range(4)]
    a = array.detach().cpu().numpy() if isinstance(array, torch.Tensor) else np.asarray(array)
    if a.shape != shape or a.dtype != np.bool_:
        raise ValueError(f"{name} must be a bool array of shape [{shape[0]},{shape[1]}], got {a.dtype} {tuple(a.shape)}")
    bits = a.reshape(4, -1, 32).astype(np.uint64) << np.arange(32, dtype=np.uint64)
    return [[int(w) for w in row] for row in bits.sum(-1)]


def check_sampling_args(temperature=None, top_k=None, top_p=None, seed=None) -> None:
    """The argument rules of sampled generation (`sample_tokens`, `generate.generate_music`); None = left at its default.
    Raises ValueError naming the argument."""
    if temperature is not None and not (_real(temperature) and math.isfinite(temperature) and temperature >= 0):
        raise ValueError(f"temperature must be a finite number >= 0, got {temperature!r}")
    if top_k is not None and not (_integer(top_k) and top_k >= 1):
        raise ValueError(f"top_k must be an int >= 1, got {top_k!r}")
    if top_p is not None and not (_real(top_p) and 0 < top_p <= 1):
        raise ValueError(f"top_p must be a number in (0, 1], got {top_p!r}")
    if seed is not None and not (_integer(seed) and 0 <= seed < 1 << 32):
        raise ValueError(f"seed must be an int in [0, 2^32), got {seed!r}")


def sample_tokens(c_logits: torch.Tensor, temperature: float = 1.0, top_k: Optional[int] = None,
                  top_p: Optional[float] = None, seed: int = 0) -> torch.Tensor:
    """`pm_sample_tokens` ("sampled generation" in include/polyphemus_hip.h): the pitch and the duration token of every
    (node, slot) row of `c_logits` [N,15,230], drawn at `temperature` from the `top_k` best tokens and / or the `top_p`
    nucleus of each head (None = filter off; temperature 0 = arg-max).  A pure function of the logits and `seed`.
    Returns int32 [N,15,2]."""
    check_sampling_args(temperature, top_k, top_p, seed)
    _chk(c_logits, F32, "c_logits")
    if c_logits.dim() != 3 or c_logits.shape[1:] != (C.MAX_SIMU_TOKENS - 1, C.D_TOKEN_PAIR):
        raise ValueError("c_logits must be [N,15,230]")
    N = c_logits.shape[0]
    tokens = torch.empty(N, C.MAX_SIMU_TOKENS - 1, 2, dtype=I32, device=c_logits.device)
    if N:
        call("pm_sample_tokens", ptr(c_logits), N * (C.MAX_SIMU_TOKENS - 1), float(temperature),
             0 if top_k is None else min(int(top_k), 1 << 30), 1.0 if top_p is None else float(top_p), int(seed), ptr(tokens),
             stream())
    return tokens


def mtp_from_tokens(tokens: torch.Tensor, s_tensor: torch.Tensor, check: bool = True) -> torch.Tensor:
    """`mtp_from_logits` with the one-hot rows of `tokens` (int32 [N,15,2] = pitch, duration) on the active cells instead of
    the nodes' logits: the per-head arg-max of an active cell returns its tokens, so the reference's `muspy_from_mtp`
    decodes a sampled piece unchanged.  A token outside its head's range leaves the head's columns zero.  Same `check`."""
    _chk(tokens, I32, "tokens")
    if tokens.dim() != 3 or tokens.shape[1:] != (C.MAX_SIMU_TOKENS - 1, 2):
        raise ValueError("tokens must be [N,15,2]")
    return _mtp("pm_mtp_from_tokens", tokens, "tokens", s_tensor, check)


def node_tracks(s_tensor: torch.Tensor, N: int, check: bool = True) -> torch.Tensor:
    """`pm_node_tracks`: uint8 [N], the track index (0 Drums .. 3 Strings) of every node of the binary structure `s_tensor`
    ([...,4,32], any dtype), nodes numbered in cell order as in `mtp_from_tokens`.  Entries behind the active cells are 0.
    `check` reads the active-cell count back (one host sync) and raises when it differs from `N`."""
    s, G, bn, npt = _structure_prologue(s_tensor, s_tensor.device, s_tensor.dim() >= 3, "s_tensor must be [...,4,32]")
    if not s_tensor.is_cuda:
        raise HipExtensionError(f"s_tensor lives on {s_tensor.device}: the HIP path needs device tensors (no CPU fallback)")
    N = int(N)
    if N < 0:
        raise ValueError(f"N must be >= 0, got {N}")
    out = torch.empty(N, dtype=U8, device=s.device)
    if G == 0:
        if check and N:
            raise ValueError(f"shape mismatch: s_tensor has 0 active cells, {N} nodes asked for")
        return out.zero_()
    call("pm_node_tracks", ptr(s), G, N, ptr(bn), ptr(npt), ptr(out) if N else None, stream())
    if check:
        _check_active(npt[G], N, f"{N} nodes asked for")
    return out


def node_cells(s_tensor: torch.Tensor, N: int, check: bool = True) -> torch.Tensor:
    """`pm_node_cells` ("Harmony" in include/polyphemus_hip.h): int32 [N], the cell index 128 g + 32 track + step of every node
    of the binary structure `s_tensor` ([...,4,32], any dtype; g counts the bars along the batch), nodes numbered in cell order
    as in `node_tracks`: `(node_cells >> 5) & 3` is `node_tracks`.  Entries behind the active cells are 0.  `check` reads the
    active-cell count back (one host sync) and raises when it differs from `N`."""
    s, G, bn, npt = _structure_prologue(s_tensor, s_tensor.device, s_tensor.dim() >= 3, "s_tensor must be [...,4,32]")
    if not s_tensor.is_cuda:
        raise HipExtensionError(f"s_tensor lives on {s_tensor.device}: the HIP path needs device tensors (no CPU fallback)")
    N = int(N)
    if N < 0:
        raise ValueError(f"N must be >= 0, got {N}")
    out = torch.empty(N, dtype=I32, device=s.device)
    if G == 0:
        if check and N:
            raise ValueError(f"shape mismatch: s_tensor has 0 active cells, {N} nodes asked for")
        return out.zero_()
    call("pm_node_cells", ptr(s), G, N, ptr(bn), ptr(npt), ptr(out) if N else None, stream())
    if check:
        _check_active(npt[G], N, f"{N} nodes asked for")
    return out


def notes_from_tokens(tokens: torch.Tensor, s_tensor: torch.Tensor, check: bool = True):
    """`pm_notes_from_tokens` ("Note events" in include/polyphemus_hip.h): the notes the reference's `muspy_from_mtp` reads out
    of `mtp_from_tokens(tokens, s_tensor)`, without the pianoroll.  `tokens` int32 [N,15,2], `s_tensor` [B,n_bars,4,32] of any
    dtype.  Returns (notes int32 [15 N,3] = time, pitch, duration; track_ptr int32 [4B+1]; totals int32 [2] = notes M, active
    cells), all on the device: the rows of (piece i, track k) are notes[track_ptr[4i+k]:track_ptr[4i+k+1]] by time, then by
    slot, and rows from M on are not written.  `check` reads `totals` back (one host sync) and raises like `mtp_from_tokens`
    when the active cells differ from N."""
    if not isinstance(tokens, torch.Tensor) or not isinstance(s_tensor, torch.Tensor):
        raise ValueError("tokens and s_tensor must be tensors")
    if tokens.dtype != I32 or tokens.dim() != 3 or tokens.shape[1:] != (C.MAX_SIMU_TOKENS - 1, 2):
        raise ValueError(f"tokens must be int32 [N,15,2], got {tokens.dtype} {tuple(tokens.shape)}")
    s, G, bn, npt, seg_count, seg_ptr = _structure_prologue(
        s_tensor, tokens.device, s_tensor.dim() == 4 and 0 not in s_tensor.shape[:2],
        f"s_tensor must be [B,n_bars,4,32] with B, n_bars >= 1, got {tuple(s_tensor.shape)}", segments=True)
    for t, name in ((tokens, "tokens"), (s_tensor, "s_tensor")):
        if not t.is_cuda:
            raise HipExtensionError(f"{name} lives on {t.device}: the HIP path needs device tensors (no CPU fallback)")
    if s_tensor.device != tokens.device:
        raise ValueError(f"s_tensor lives on {s_tensor.device}, tokens on {tokens.device}")
    tokens = tokens.contiguous()
    B, n_bars = s_tensor.shape[:2]
    N, dev = tokens.shape[0], tokens.device
    cap = (C.MAX_SIMU_TOKENS - 1) * N
    notes = torch.empty(cap, 3, dtype=I32, device=dev)
    track_ptr, totals = torch.empty(4 * B + 1, dtype=I32, device=dev), torch.empty(2, dtype=I32, device=dev)
    call("pm_notes_from_tokens", ptr(tokens) if N else None, ptr(s), G, n_bars, N, ptr(seg_count), ptr(seg_ptr), ptr(bn), ptr(npt),
         ptr(notes) if N else None, cap, ptr(track_ptr), ptr(totals), stream())
    if check:
        _check_active(totals[1], N, f"tokens has {N} nodes")
    return notes, track_ptr, totals


def tokens_from_notes(notes: torch.Tensor, track_ptr: torch.Tensor, n_bars: int, check: bool = True):
    """`pm_tokens_from_notes` ("Notes in" in include/polyphemus_hip.h), the inverse of `notes_from_tokens`: pieces held as note
    events become what the encoder consumes.  `notes` int32 [M,3] rows (time, pitch, duration) and `track_ptr` int32 [4B+1]
    are the `NoteBatch` layout (rows behind track_ptr[4B] are ignored); a piece is `n_bars` bars of 32 steps.  Returns
    (s_tensor fp32 [B n_bars,4,32] 0/1, tokens int32 [N,16,2], info): the nodes are the active cells in cell order, the rows
    `graph_build(s_tensor, n_bars)` numbers; a cell keeps its first 14 notes in row order and a bar without a note gets cell
    [0,0] with none (preprocess.py:118-157, data.py:148-153).  ONE host read brings the node count N, which sizes `tokens`,
    and the input check with it: info = {"dropped": notes that found no slot, "out_of_range", "out_of_order",
    "bad_track_ptr", "num_nodes"}.  With `check` rows whose time is outside the piece or out of order and bad `track_ptr`
    entries raise ValueError with their count; without it they are only counted (the kernels never follow them)."""
    for t, name in ((notes, "notes"), (track_ptr, "track_ptr")):
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{name} must be a tensor, got {type(t).__name__}")
    if notes.dtype != I32 or notes.dim() != 2 or notes.shape[1] != 3:
        raise ValueError(f"notes must be int32 [M,3], got {notes.dtype} {tuple(notes.shape)}")
    if track_ptr.dtype != I32 or track_ptr.dim() != 1 or track_ptr.shape[0] < 5 or track_ptr.shape[0] % 4 != 1:
        raise ValueError(f"track_ptr must be int32 [4B+1] with B >= 1, got {track_ptr.dtype} {tuple(track_ptr.shape)}")
    if not (_integer(n_bars) and n_bars >= 1):
        raise ValueError(f"n_bars must be an int >= 1, got {n_bars!r}")
    for t, name in ((notes, "notes"), (track_ptr, "track_ptr")):
        if not t.is_cuda:
            raise HipExtensionError(f"{name} lives on {t.device}: the HIP path needs device tensors (no CPU fallback)")
    if track_ptr.device != notes.device:
        raise ValueError(f"track_ptr lives on {track_ptr.device}, notes on {notes.device}")
    notes, track_ptr, n_bars = notes.contiguous(), track_ptr.contiguous(), int(n_bars)
    B, M, dev = track_ptr.shape[0] // 4, notes.shape[0], notes.device
    G = B * n_bars
    cap = min(M + G, 128 * G)                        # every node but an empty bar's has a note of its own
    s = torch.empty(G, 4, 32, dtype=F32, device=dev)
    buf = torch.empty(cap, C.MAX_SIMU_TOKENS, 2, dtype=I32, device=dev)
    scratch, status = torch.empty(3 * G + 1 + 12 * B + 5, dtype=I32, device=dev).split([3 * G + 1 + 12 * B, 5])
    call("pm_tokens_from_notes", ptr(notes) if M else None, ptr(track_ptr), B, n_bars, M, ptr(s), ptr(buf), cap, ptr(scratch),
         ptr(status), stream())
    out_of_range, out_of_order, bad_ptr, dropped, N = status.tolist()             # the one host read
    if check or N > cap:
        for count, what in ((bad_ptr, f"track_ptr: {{}} bad entries (below the entry before them, outside [0, {M}] or, the "
                                      "first, not 0)"),
                            (out_of_range, f"notes: {{}} rows out of range (a time outside [0, {32 * n_bars}))"),
                            (out_of_order, "notes: {} rows out of order (a time above the next row's of the same track)")):
            if count:
                raise ValueError(what.format(count))
    if N > cap:                                      # (only input that breaks the contract gets here)
        raise ValueError(f"notes: {N} active cells out of {M} rows and {G} bars")
    tokens = buf if N == cap else buf[:N].clone()    # (the clone lets the worst-case buffer go)
    return s, tokens, dict(dropped=dropped, out_of_range=out_of_range, out_of_order=out_of_order, bad_track_ptr=bad_ptr,
                           num_nodes=N)


def check_region(region, B: int, n_bars: int) -> np.ndarray:
    """The region of an infill ("Infill" in include/polyphemus_hip.h) as a contiguous bool numpy array: `region` is a bool
    array-like or bool tensor [n_bars,4,32] (one mask for all pieces) or [B,n_bars,4,32] (one per piece), True = the model
    rewrites the cell.  Anything else raises ValueError, before a device is touched."""
    if isinstance(region, torch.Tensor):
        if region.dtype != torch.bool:
            raise ValueError(f"region must be a bool array [n_bars,4,32] or [B,n_bars,4,32], got a {region.dtype} tensor")
        a = region.detach().cpu().numpy()
    else:
        try:
            a = np.asarray(region)
        except Exception:
            a = np.empty(0, np.object_)
    if a.dtype != np.bool_ or tuple(a.shape) not in ((n_bars, 4, 32), (B, n_bars, 4, 32)):
        raise ValueError(f"region must be a bool array [n_bars,4,32] = [{n_bars},4,32] or [B,n_bars,4,32] = "
                         f"[{B},{n_bars},4,32], got {a.dtype} {tuple(a.shape)}")
    return np.ascontiguousarray(a)


def _infill_args(named, region):
    """The checks `infill_structure` and `infill_tokens` share: every (tensor, name, dtype, trailing shape) of `named` is a
    tensor of that dtype and shape (ValueError), on the device (HipExtensionError), all on one device (ValueError); the
    structures agree in their bar count G; `region` is bool / uint8 [R,4,32] or [B,n_bars,4,32] with R = G or a divisor of
    G, a tensor on that device or an array-like that is uploaded.  Returns (contiguous tensors, region uint8 [R,4,32], G, R)."""
    for t, name, dtype, tail in named:
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{name} must be a tensor, got {type(t).__name__}")
        if t.dtype != dtype or t.dim() < len(tail) + 1 or tuple(t.shape[-len(tail):]) != tail:
            raise ValueError(f"{name} must be {dtype} [...,{','.join(map(str, tail))}], got {t.dtype} {tuple(t.shape)}")
    if not isinstance(region, torch.Tensor):
        region = np.asarray(region)
        if region.dtype != np.bool_:
            raise ValueError(f"region must be a bool array [R,4,32], got {region.dtype} {tuple(region.shape)}")
        region = torch.from_numpy(np.ascontiguousarray(region))
        if named[0][0].is_cuda:
            region = region.to(named[0][0].device)
    if region.dtype not in (torch.bool, U8) or region.dim() < 3 or tuple(region.shape[-2:]) != (4, 32):
        raise ValueError(f"region must be bool [R,4,32] or [B,n_bars,4,32], got {region.dtype} {tuple(region.shape)}")
    structures = [t for t, _, _, tail in named if tail == (4, 32)]
    G, R = structures[0].numel() // 128, region.numel() // 128
    for t, name, _, tail in named:
        if tail == (4, 32) and t.numel() != 128 * G:
            raise ValueError(f"{name} holds {t.numel() // 128} bars, {named[0][1]} holds {G}")
    if G == 0 or R == 0 or G % R != 0:
        raise ValueError(f"region holds {R} bars: it must hold the structures' {G} bars or a divisor of them, and at least one")
    for t, name in [(t, name) for t, name, _, _ in named] + [(region, "region")]:
        if not t.is_cuda:
            raise HipExtensionError(f"{name} lives on {t.device}: the HIP path needs device tensors (no CPU fallback)")
    for t, name in [(t, name) for t, name, _, _ in named[1:]] + [(region, "region")]:
        if t.device != named[0][0].device:
            raise ValueError(f"{name} lives on {t.device}, {named[0][1]} on {named[0][0].device}")
    region = region.contiguous()
    return [t.contiguous() for t, _, _, _ in named], (region.view(U8) if region.dtype == torch.bool else region), G, R


def infill_structure(s_in: torch.Tensor, s_model: torch.Tensor, region):
    """`pm_infill_structure` ("Infill" in include/polyphemus_hip.h): the structure of an infill.  `s_in` fp32 [G,4,32] 0/1 is
    the input's structure (`tokens_from_notes`), `s_model` bool or uint8 [...,4,32] with G bars the model's
    (`binary_from_logits`, `sample_structure`), `region` bool [R,4,32] or [B,n_bars,4,32] (R = G or a divisor of G: bar g reads
    row g % R).  A cell is on iff (region ? s_model : s_in); a bar that comes out empty gets cell [0,0].  Returns (bool
    [G,4,32], bar_forced int32 [G]: 1 where [0,0] was switched on).  One launch, nothing is read back."""
    if isinstance(s_model, torch.Tensor) and s_model.dtype == torch.bool:
        s_model = s_model.view(U8) if s_model.is_contiguous() else s_model.contiguous().view(U8)
    (s_in, s_model), region, G, R = _infill_args([(s_in, "s_in", F32, (4, 32)), (s_model, "s_model", U8, (4, 32))], region)
    out = torch.empty(G, 4, 32, dtype=U8, device=s_in.device)
    bar_forced = torch.empty(G, dtype=I32, device=s_in.device)
    call("pm_infill_structure", ptr(s_in), ptr(s_model), ptr(region), G, R, None, ptr(out), ptr(bar_forced), stream())
    return out.view(torch.bool), bar_forced


def infill_tokens(s_in: torch.Tensor, s_out: torch.Tensor, region, tokens_in: torch.Tensor, tokens: torch.Tensor,
                  bar_forced: Optional[torch.Tensor] = None) -> torch.Tensor:
    """`pm_infill_tokens` ("Infill" in include/polyphemus_hip.h): the kept cells' tokens put back, IN PLACE.  `s_in` fp32
    [G,4,32] and `tokens_in` int32 [N_in,16,2] are the input (`tokens_from_notes`), `s_out` fp32 [G,4,32] the merged structure
    after the decoder's graph build, `tokens` int32 [N,15,2] (contiguous) the drawn tokens of its nodes, `region` as for
    `infill_structure`.  A node outside the region takes the 15 slots behind the SOS of the input's node of its cell, or the
    chord of a cell without a note where the input has none; nodes inside the region stay as drawn.  Returns status int32 [5]
    on the device: active cells of s_out, of s_in, kept nodes, kept nodes without a source, bars forced (the sum of
    `bar_forced`, int32 [G] from `infill_structure`; None counts none).  Nothing is read back: a caller that has not
    checked N against s_out's cells compares status[0] with it."""
    named = [(s_in, "s_in", F32, (4, 32)), (s_out, "s_out", F32, (4, 32)), (tokens_in, "tokens_in", I32, (C.MAX_SIMU_TOKENS, 2)),
             (tokens, "tokens", I32, (C.MAX_SIMU_TOKENS - 1, 2))]
    for t, name, _, tail in named[2:]:
        if isinstance(t, torch.Tensor) and t.dim() != 3:
            raise ValueError(f"{name} must be int32 [N,{tail[0]},2], got {t.dtype} {tuple(t.shape)}")
    if bar_forced is not None and not (isinstance(bar_forced, torch.Tensor) and bar_forced.dtype == I32 and bar_forced.dim() == 1):
        raise ValueError("bar_forced must be an int32 tensor [G]")
    if isinstance(tokens, torch.Tensor) and not tokens.is_contiguous():
        raise ValueError("tokens must be contiguous: it is written in place")
    (s_in, s_out, tokens_in, tokens), region, G, R = _infill_args(named, region)
    if bar_forced is not None:
        if bar_forced.shape[0] != G or bar_forced.device != s_in.device:
            raise ValueError(f"bar_forced must be int32 [G = {G}] on {s_in.device}, got [{bar_forced.shape[0]}] on {bar_forced.device}")
        bar_forced = bar_forced.contiguous()
    N_in, N, dev = tokens_in.shape[0], tokens.shape[0], s_in.device
    scratch, status = torch.empty(6 * G + 2 + 5, dtype=I32, device=dev).split([6 * G + 2, 5])   # PM_INFILL_SCRATCH(G)
    call("pm_infill_tokens", ptr(s_in), ptr(s_out), ptr(region), G, R, ptr(tokens_in) if N_in else None, N_in,
         ptr(tokens) if N else None, N, ptr(bar_forced), ptr(scratch), ptr(status), stream())
    return status


NOTE_STAT_FIELDS = ("n_notes", "n_onsets", "pitch_min", "pitch_max", "n_pitches", "n_pitch_classes", "note_steps",
                    "sounding_steps", "poly_steps", "max_polyphony", "max_chord", "out_of_range")    # PM_NOTE_STAT_*
MAX_STAT_BARS = 64


def _note_batch_args(notes, track_ptr):
    """The checks the readers of the `NoteBatch` layout share (`tokens_from_notes`' rules): `notes` int32 [M,3] and `track_ptr`
    int32 [4B+1] tensors (ValueError), on one device (ValueError) that is a GPU (HipExtensionError).  `check_device` runs
    last, so a caller puts its own argument checks between the two."""
    for t, name in ((notes, "notes"), (track_ptr, "track_ptr")):
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{name} must be a tensor, got {type(t).__name__}")
    if notes.dtype != I32 or notes.dim() != 2 or notes.shape[1] != 3:
        raise ValueError(f"notes must be int32 [M,3], got {notes.dtype} {tuple(notes.shape)}")
    if track_ptr.dtype != I32 or track_ptr.dim() != 1 or track_ptr.shape[0] < 5 or track_ptr.shape[0] % 4 != 1:
        raise ValueError(f"track_ptr must be int32 [4B+1] with B >= 1, got {track_ptr.dtype} {tuple(track_ptr.shape)}")

    def check_device():
        for t, name in ((notes, "notes"), (track_ptr, "track_ptr")):
            if not t.is_cuda:
                raise HipExtensionError(f"{name} lives on {t.device}: the HIP path needs device tensors (no CPU fallback)")
        if track_ptr.device != notes.device:
            raise ValueError(f"track_ptr lives on {track_ptr.device}, notes on {notes.device}")
    return check_device


def note_stats(notes: torch.Tensor, track_ptr: torch.Tensor, n_bars: int, check: bool = False):
    """`pm_note_stats` ("Note statistics" in include/polyphemus_hip.h): what the pieces of the `NoteBatch` layout (`notes` int32
    [M,3], `track_ptr` int32 [4B+1], `n_bars` bars of 32 steps, at most 64) hold, counted per (piece, track) on the device in
    one launch.  A row is counted iff its time lies inside the piece, as the note the encoder would see (pitch clamped to
    0..127, duration to 1..96, cut at the end of the piece).  Returns four int32 tensors: track [4B,12] (NOTE_STAT_FIELDS),
    pitch_class [4B,12], onsets [4B,n_bars] and sounding [4B,n_bars] (bit s of word b: step 32 b + s).  Nothing is read back
    unless `check` is set: then rows outside the piece (`out_of_range`) raise ValueError with their count."""
    check_device = _note_batch_args(notes, track_ptr)
    if not (_integer(n_bars) and 1 <= n_bars <= MAX_STAT_BARS):
        raise ValueError(f"n_bars must be an int in [1, {MAX_STAT_BARS}], got {n_bars!r}")
    check_device()
    notes, track_ptr, n_bars = notes.contiguous(), track_ptr.contiguous(), int(n_bars)
    B, M, dev = track_ptr.shape[0] // 4, notes.shape[0], notes.device
    nf = len(NOTE_STAT_FIELDS)
    track, pitch_class = torch.empty(4 * B, nf, dtype=I32, device=dev), torch.empty(4 * B, 12, dtype=I32, device=dev)
    onsets, sounding = torch.empty(4 * B, n_bars, dtype=I32, device=dev), torch.empty(4 * B, n_bars, dtype=I32, device=dev)
    call("pm_note_stats", ptr(notes) if M else None, ptr(track_ptr), B, n_bars, M, ptr(track), ptr(pitch_class), ptr(onsets),
         ptr(sounding), stream())
    if check:
        bad = int(track[:, nf - 1].sum().item())                 # the one host read
        if bad:
            raise ValueError(f"notes: {bad} rows out of range (a time outside [0, {32 * n_bars}))")
    return track, pitch_class, onsets, sounding


SEG_STEPS = (1, 2, 4, 8, 16, 32)                 # the segment lengths of a chromagram, and the sets per bar of a harmony


def note_chroma(notes: torch.Tensor, track_ptr: torch.Tensor, n_bars: int, seg_steps: int = 32) -> torch.Tensor:
    """`pm_note_chroma` ("Harmony" in include/polyphemus_hip.h): the chromagram of the pieces of the `NoteBatch` layout (`notes`
    int32 [M,3], `track_ptr` int32 [4B+1], `n_bars` bars of 32 steps, at most 64), int32 [4B, S, 12] with S = 32 n_bars /
    `seg_steps` (1, 2, 4, 8, 16 or 32): entry [track, s, c] counts the (note, step) pairs of pitch class c sounding in segment
    s.  A row counts as in `note_stats` (a time inside the piece, the pitch clamped to 0..127, the duration to 1..96 and cut at
    the piece's end).  One launch, nothing is read back; bit-identical from call to call."""
    check_device = _note_batch_args(notes, track_ptr)
    if not (_integer(n_bars) and 1 <= n_bars <= MAX_STAT_BARS):
        raise ValueError(f"n_bars must be an int in [1, {MAX_STAT_BARS}], got {n_bars!r}")
    if not (_integer(seg_steps) and seg_steps in SEG_STEPS):
        raise ValueError(f"seg_steps must be one of {SEG_STEPS}, got {seg_steps!r}")
    check_device()
    notes, track_ptr, n_bars, seg_steps = notes.contiguous(), track_ptr.contiguous(), int(n_bars), int(seg_steps)
    B, M = track_ptr.shape[0] // 4, notes.shape[0]
    chroma = torch.empty(4 * B, 32 * n_bars // seg_steps, 12, dtype=I32, device=notes.device)
    call("pm_note_chroma", ptr(notes) if M else None, ptr(track_ptr), B, M, n_bars, seg_steps, ptr(chroma), stream())
    return chroma


def notes_select(notes: torch.Tensor, track_ptr: torch.Tensor, index, check: bool = True):
    """`pm_notes_select` ("Note statistics" in include/polyphemus_hip.h): the pieces `index[0..K)` of the `NoteBatch` layout
    (`notes` int32 [M,3], `track_ptr` int32 [4B+1]), in that order, without leaving the device.  `index` is an int32 or int64
    tensor [K] or a list of ints, K >= 1, its entries in [0, B) and distinct.  Returns (notes int32 [M,3], track_ptr int32
    [4K+1], totals int32 [2] = rows M', cells; status int32 [2] = entries out of range, entries that repeat an earlier one):
    the new notes buffer has the input's size, which distinct entries cannot exceed, and rows from M' on are not written.  An
    entry that is counted in `status` gives an empty piece.  `check` reads `status` back (one host sync) and raises ValueError
    with the counts; without it nothing is read back."""
    check_device = _note_batch_args(notes, track_ptr)
    if isinstance(index, torch.Tensor):
        if index.dtype not in (I32, I64) or index.dim() != 1 or index.shape[0] < 1:
            raise ValueError(f"index must be an int32 or int64 tensor [K] with K >= 1, got {index.dtype} {tuple(index.shape)}")
    elif isinstance(index, (list, tuple)) and len(index) >= 1 and all(_integer(v) and -(1 << 31) <= v < (1 << 31) for v in index):
        index = torch.tensor([int(v) for v in index], dtype=I32)
        if notes.is_cuda:
            index = index.to(notes.device)
    else:
        raise ValueError(f"index must be an int32 or int64 tensor [K] or a non-empty list of ints, got {index!r}")
    check_device()
    if index.device != notes.device:
        raise ValueError(f"index lives on {index.device}, notes on {notes.device}")
    B, M, K, dev = track_ptr.shape[0] // 4, notes.shape[0], index.shape[0], notes.device
    if index.dtype == I64:                                       # (an entry beyond int32 is out of range either way)
        index = index.clamp(-1, B).to(I32)
    notes, track_ptr, index = notes.contiguous(), track_ptr.contiguous(), index.contiguous()
    out = torch.empty(M, 3, dtype=I32, device=dev)
    out_ptr = torch.empty(4 * K + 1, dtype=I32, device=dev)
    n_scratch = B + 16 * K                                       # PM_SELECT_SCRATCH(B, K)
    scratch, totals, status = torch.empty(n_scratch + 4, dtype=I32, device=dev).split([n_scratch, 2, 2])
    call("pm_notes_select", ptr(notes) if M else None, ptr(track_ptr), B, M, ptr(index), K, ptr(out) if M else None, M,
         ptr(out_ptr), ptr(totals), ptr(scratch), ptr(status), stream())
    totals, status = totals.clone(), status.clone()              # (lets the scratch go)
    if check:
        out_of_range, repeated = status.tolist()                 # the one host read
        if out_of_range or repeated:
            raise ValueError(f"index: {out_of_range} entries outside [0, {B}), {repeated} entries that repeat an earlier one")
    return out, out_ptr, totals, status


MAX_RULE_BARS = 64


def notes_splice(notes: torch.Tensor, track_ptr: torch.Tensor, src_bars: int, segments: torch.Tensor, seg_ptr: torch.Tensor,
                 out_bars: int, shift: Optional[torch.Tensor] = None, silence_rule: bool = False, capacity: Optional[int] = None,
                 check: bool = True):
    """`pm_notes_splice` ("Note splicing" in include/polyphemus_hip.h): bar ranges of the pieces of the `NoteBatch` layout
    (`notes` int32 [M,3], `track_ptr` int32 [4B+1], pieces of `src_bars` bars) copied into bar ranges of K new pieces of
    `out_bars` bars, without leaving the device.  `segments` int32 [S,4] holds rows (src_piece, src_bar, out_bar, bars) and
    `seg_ptr` int32 [K+1] the segments of every output piece; a row goes along by its onset, rebased, in the source's order.
    `shift` int32 [K] transposes the tracks 1..3 of every output piece (pitches clamped to 0..127 before and after), None
    leaves the pitches alone; `silence_rule` asks for the reference's silence filters (out_bars <= 64) in `keep`; `capacity`
    is the rows of the new notes buffer, M by default.  Returns (notes int32 [capacity,3], track_ptr int32 [4K+1], totals
    int32 [2] = rows needed, cells; keep int32 [K]; status int32 [4] = segments not followed, bad seg_ptr entries, rows beyond
    the capacity, 0).  `check` reads `status` back (one host sync) and raises ValueError with the counts; without it
    nothing is read back and what is counted was not followed."""
    check_device = _note_batch_args(notes, track_ptr)
    if not (_integer(src_bars) and 1 <= src_bars <= 0x7fffffff // 32):
        raise ValueError(f"src_bars must be an int >= 1, got {src_bars!r}")
    if not (_integer(out_bars) and 1 <= out_bars <= 0x7fffffff // 32):
        raise ValueError(f"out_bars must be an int >= 1, got {out_bars!r}")
    if not isinstance(segments, torch.Tensor) or segments.dtype != I32 or segments.dim() != 2 or segments.shape[1] != 4:
        raise ValueError("segments must be an int32 tensor [S,4], got "
                         + (f"{segments.dtype} {tuple(segments.shape)}" if isinstance(segments, torch.Tensor) else type(segments).__name__))
    if not isinstance(seg_ptr, torch.Tensor) or seg_ptr.dtype != I32 or seg_ptr.dim() != 1 or seg_ptr.shape[0] < 2:
        raise ValueError("seg_ptr must be an int32 tensor [K+1] with K >= 1, got "
                         + (f"{seg_ptr.dtype} {tuple(seg_ptr.shape)}" if isinstance(seg_ptr, torch.Tensor) else type(seg_ptr).__name__))
    K, S, M = seg_ptr.shape[0] - 1, segments.shape[0], notes.shape[0]
    if shift is not None and not (isinstance(shift, torch.Tensor) and shift.dtype == I32 and tuple(shift.shape) == (K,)):
        raise ValueError(f"shift must be None or an int32 tensor [K = {K}], got "
                         + (f"{shift.dtype} {tuple(shift.shape)}" if isinstance(shift, torch.Tensor) else type(shift).__name__))
    if not isinstance(silence_rule, (bool, np.bool_)):
        raise ValueError(f"silence_rule must be a bool, got {silence_rule!r}")
    if silence_rule and out_bars > MAX_RULE_BARS:
        raise ValueError(f"silence_rule needs out_bars <= {MAX_RULE_BARS}, got {out_bars}")
    if capacity is None:
        capacity = M
    if not (_integer(capacity) and 0 <= capacity <= 0x7fffffff // 3):
        raise ValueError(f"capacity must be an int in [0, {0x7fffffff // 3}], got {capacity!r}")
    check_device()
    for t, name in ((segments, "segments"), (seg_ptr, "seg_ptr"), (shift, "shift")):
        if t is not None and t.device != notes.device:
            raise ValueError(f"{name} lives on {t.device}, notes on {notes.device}")
    B, cap, dev = track_ptr.shape[0] // 4, int(capacity), notes.device
    notes, track_ptr, segments, seg_ptr = notes.contiguous(), track_ptr.contiguous(), segments.contiguous(), seg_ptr.contiguous()
    shift = None if shift is None else shift.contiguous()
    out = torch.empty(cap, 3, dtype=I32, device=dev)
    out_ptr, keep = torch.empty(4 * K + 1, dtype=I32, device=dev), torch.empty(K, dtype=I32, device=dev)
    n_scratch = 24 * K                                           # PM_SPLICE_SCRATCH(K, S)
    scratch, totals, status = torch.empty(n_scratch + 6, dtype=I32, device=dev).split([n_scratch, 2, 4])
    call("pm_notes_splice", ptr(notes) if M else None, ptr(track_ptr), B, int(src_bars), M, ptr(segments) if S else None, S,
         ptr(seg_ptr), K, int(out_bars), ptr(shift), int(bool(silence_rule)), ptr(out) if cap else None, cap, ptr(out_ptr),
         ptr(totals), ptr(keep), ptr(scratch), ptr(status), stream())
    totals, status = totals.clone(), status.clone()              # (lets the scratch go)
    if check:
        bad_seg, bad_ptr, excess, _ = status.tolist()            # the one host read
        if bad_seg or bad_ptr or excess:
            raise ValueError(f"segments: {bad_seg} not followed (a piece outside [0, {B}), a bar range outside the source's "
                             f"{src_bars} or the output's {out_bars} bars, or an output range in front of the end of the one "
                             f"before); seg_ptr: {bad_ptr} bad entries (outside [0, {S}] or below the entry before them); "
                             f"notes: {excess} rows beyond the capacity of {cap}")
    return out, out_ptr, totals, keep, status


def _on_device(named) -> None:
    """HipExtensionError for the first of (tensor, name) that is no device tensor, ValueError when they do not share a device."""
    for t, name in named:
        if not t.is_cuda:
            raise HipExtensionError(f"{name} lives on {t.device}: the HIP path needs device tensors (no CPU fallback)")
    for t, name in named[1:]:
        if t.device != named[0][0].device:
            raise ValueError(f"{name} lives on {t.device}, {named[0][1]} on {named[0][0].device}")


def score_tokens(c_logits: torch.Tensor, tokens: torch.Tensor, s_tensor: torch.Tensor, check: bool = True,
                 return_verdict: bool = False):
    """`pm_score_tokens` ("Scores" in include/polyphemus_hip.h): the log-likelihood of `tokens` under `c_logits` [N,15,230],
    per bar and track of `s_tensor` [B,n_bars,4,32] (any dtype), whose active cells are the nodes in cell order.  `tokens` is
    int32 [N,15,2] (the layout of `sample_tokens`) or [N,16,2] (`tokens_from_notes`, `BarGraphBatch.tokens`: slot 0, the SOS,
    is no target); a PAD target adds nothing.  Returns (logp float64 [B,n_bars,4,2] = the summed pitch and duration
    log-probabilities; counts int32 [B,n_bars,4,6] = nodes, pitch targets, duration targets, pitch hits, duration hits, note
    hits; row_logp float32 [N,15,2]), with `return_verdict` also the rows' verdict bytes uint8 [N,15] (bit 0 pitch hit, 1
    duration hit, 2 pitch target, 3 duration target).  Bit-identical from call to call, and a bar's numbers do not depend on
    the rest of the batch.  `check` reads the active-cell count back (one host sync) and raises like `mtp_from_tokens` when it
    differs from N."""
    for t, name in ((c_logits, "c_logits"), (tokens, "tokens"), (s_tensor, "s_tensor")):
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{name} must be a tensor, got {type(t).__name__}")
    S = C.MAX_SIMU_TOKENS - 1
    if c_logits.dtype != F32 or c_logits.dim() != 3 or c_logits.shape[1:] != (S, C.D_TOKEN_PAIR):
        raise ValueError(f"c_logits must be float32 [N,15,230], got {c_logits.dtype} {tuple(c_logits.shape)}")
    if tokens.dtype != I32 or tokens.dim() != 3 or tokens.shape[1] not in (S, S + 1) or tokens.shape[2] != 2:
        raise ValueError(f"tokens must be int32 [N,15,2] or [N,16,2], got {tokens.dtype} {tuple(tokens.shape)}")
    if tokens.shape[0] != c_logits.shape[0]:
        raise ValueError(f"tokens has {tokens.shape[0]} nodes, c_logits {c_logits.shape[0]}")
    s, G, bn, npt = _structure_prologue(
        s_tensor, c_logits.device, s_tensor.dim() == 4 and 0 not in s_tensor.shape[:2],
        f"s_tensor must be [B,n_bars,4,32] with B, n_bars >= 1, got {tuple(s_tensor.shape)}")
    _on_device([(c_logits, "c_logits"), (tokens, "tokens"), (s_tensor, "s_tensor")])
    c_logits, tokens = c_logits.contiguous(), tokens.contiguous()
    B, n_bars = s_tensor.shape[:2]
    N, dev = c_logits.shape[0], c_logits.device
    row_logp, verdict = torch.empty(N, S, 2, dtype=F32, device=dev), torch.empty(N, S, dtype=U8, device=dev)
    logp, counts = torch.empty(B, n_bars, 4, 2, dtype=F64, device=dev), torch.empty(B, n_bars, 4, 6, dtype=I32, device=dev)
    call("pm_score_tokens", ptr(c_logits) if N else None, ptr(tokens) if N else None, tokens.shape[1], ptr(s), G, N, ptr(bn),
         ptr(npt), ptr(row_logp) if N else None, ptr(verdict) if N else None, ptr(logp), ptr(counts), stream())
    if check:
        _check_active(npt[G], N, f"c_logits has {N} nodes")
    return (logp, counts, row_logp, verdict) if return_verdict else (logp, counts, row_logp)


def score_structure(s_logits: torch.Tensor, s_tensor: torch.Tensor):
    """`pm_score_structure` ("Scores" in include/polyphemus_hip.h): the Bernoulli log-likelihood of the cells of `s_tensor`
    [B,n_bars,4,32] (any dtype; on = non-zero) under `s_logits` (float32, the same shape), per bar and track.  Returns (logp
    float64 [B,n_bars,4]; counts int32 [B,n_bars,4,4] = targets on, predictions on, true positives, cells that agree, the
    prediction being `structure_metrics`').  One launch, no host read; bit-identical from call to call."""
    for t, name in ((s_logits, "s_logits"), (s_tensor, "s_tensor")):
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{name} must be a tensor, got {type(t).__name__}")
    if s_tensor.dim() != 4 or 0 in s_tensor.shape[:2] or s_tensor.shape[2:] != (4, 32):
        raise ValueError(f"s_tensor must be [B,n_bars,4,32] with B, n_bars >= 1, got {tuple(s_tensor.shape)}")
    if s_logits.dtype != F32 or s_logits.shape != s_tensor.shape:
        raise ValueError(f"s_logits must be float32 {tuple(s_tensor.shape)}, got {s_logits.dtype} {tuple(s_logits.shape)}")
    _on_device([(s_logits, "s_logits"), (s_tensor, "s_tensor")])
    s_logits, s = s_logits.contiguous(), s_tensor.to(F32).contiguous()
    B, n_bars = s_tensor.shape[:2]
    logp = torch.empty(B, n_bars, 4, dtype=F64, device=s_logits.device)
    counts = torch.empty(B, n_bars, 4, 4, dtype=I32, device=s_logits.device)
    call("pm_score_structure", ptr(s_logits), ptr(s), B * n_bars, ptr(logp), ptr(counts), stream())
    return logp, counts


def check_chord_args(temperature=None, top_k=None, top_p=None, seed=None, min_notes=1, max_notes=14, allowed_pitches=None,
                     c_logits=None, node_track=None):
    """The argument rules of chord-aware sampling (`sample_chords`, `generate.generate_music(chord_rules=...)`): raises
    ValueError naming the argument.  `temperature` is a number or a pair (pitch, duration); `min_notes` / `max_notes` an int
    or four ints (Drums, Bass, Guitar, Strings) with 0 <= min_notes <= max_notes and 1 <= max_notes <= 14;
    `allowed_pitches` None or a bool array-like [4,128]; `node_track`, when given, uint8 [N] on the device of `c_logits`.
    Returns ((T_pitch, T_duration), min_notes [4], max_notes [4], pitch_mask: 4 x 4 words of 32 bits)."""
    if temperature is None:
        temperature = 1.0
    pair = tuple(temperature) if isinstance(temperature, (tuple, list)) else (temperature, temperature)
    if len(pair) != 2 or not all(_real(v) and math.isfinite(v) and v >= 0 for v in pair):
        raise ValueError(f"temperature must be a finite number >= 0 or a pair (pitch, duration) of them, got {temperature!r}")
    check_sampling_args(None, top_k, top_p, seed)
    mx = _four(max_notes, "max_notes")
    if not all(1 <= a <= C.MAX_SIMU_TOKENS - 2 for a in mx):
        raise ValueError(f"max_notes must be in [1, {C.MAX_SIMU_TOKENS - 2}], got {max_notes!r}")
    mn = _four(min_notes, "min_notes")
    if not all(0 <= a <= b for a, b in zip(mn, mx)):
        raise ValueError(f"min_notes must satisfy 0 <= min_notes <= max_notes = {max_notes!r}, got {min_notes!r}")
    words = _mask_words(allowed_pitches, (4, 128), "allowed_pitches")
    if node_track is not None:
        if not isinstance(node_track, torch.Tensor) or node_track.dtype != U8 or node_track.dim() != 1 or not node_track.is_contiguous():
            raise ValueError("node_track must be a contiguous uint8 tensor [N]")
        if c_logits is not None and (node_track.shape[0] != c_logits.shape[0] or node_track.device != c_logits.device):
            raise ValueError(f"node_track must be uint8 [N = {c_logits.shape[0]}] on {c_logits.device}, got "
                             f"[{node_track.shape[0]}] on {node_track.device}")
    return (float(pair[0]), float(pair[1])), mn, mx, words


def sample_chords(c_logits: torch.Tensor, node_track: torch.Tensor, temperature=1.0, top_k: Optional[int] = None,
                  top_p: Optional[float] = None, seed: int = 0, min_notes=1, max_notes=14, allowed_pitches=None):
    """`pm_sample_chords` (chord-aware sampling, "sampled generation" in include/polyphemus_hip.h): every node's 15 slots
    drawn in order as notes, one EOS, then PAD.  A pitch is drawn from the pitches `allowed_pitches` ([4,128] bool, None =
    all) gives the node's track (`node_track`, uint8 [N], see `node_tracks`) that the chord does not hold yet, while it has
    fewer than `max_notes` notes; the EOS from `min_notes` notes on; the duration among 0..95.  `temperature` is a number or a
    pair (pitch, duration), 0 = arg-max over the candidates; `top_k` / `top_p` apply to the candidates.  A pure function of
    the logits, the rules and `seed`.  Returns (tokens int32 [N,15,2], note_count int32 [N])."""
    from ._lib import PmChordRules
    _chk(c_logits, F32, "c_logits")
    if c_logits.dim() != 3 or c_logits.shape[1:] != (C.MAX_SIMU_TOKENS - 1, C.D_TOKEN_PAIR):
        raise ValueError("c_logits must be [N,15,230]")
    temps, mn, mx, words = check_chord_args(temperature, top_k, top_p, seed, min_notes, max_notes, allowed_pitches,
                                            c_logits=c_logits, node_track=node_track)
    if node_track is None:
        raise ValueError("node_track is None")
    N = c_logits.shape[0]
    tokens = torch.empty(N, C.MAX_SIMU_TOKENS - 1, 2, dtype=I32, device=c_logits.device)
    note_count = torch.empty(N, dtype=I32, device=c_logits.device)
    if N:
        rules = PmChordRules()
        rules.temperature[0], rules.temperature[1] = temps
        rules.top_k = 0 if top_k is None else min(int(top_k), 1 << 30)
        rules.top_p = 1.0 if top_p is None else float(top_p)
        for k in range(4):
            rules.min_notes[k], rules.max_notes[k] = mn[k], mx[k]
            for w in range(4):
                rules.pitch_mask[k][w] = words[k][w]
        call("pm_sample_chords", ptr(c_logits), ptr(node_track), N, ctypes.addressof(rules), int(seed), ptr(tokens),
             ptr(note_count), stream())
    return tokens, note_count


TRACK_NAMES = ("Drums", "Bass", "Guitar", "Strings")            # constants.py:5


def check_harmony_args(sets, tracks=("Bass", "Guitar", "Strings"), empty="free", B=None, n_bars=None):
    """The argument rules of a harmony (`generate.Harmony`, `sample_chords_at`): raises ValueError naming the argument, before
    anything touches the device.  `sets` is an int tensor or array-like [n_bars,S] (shared by all pieces) or [B,n_bars,S] with
    S in {1, 2, 4, 8, 16, 32} sets per bar and values in [0, 4096): bit c set = pitch class c may sound.  The values of a host
    array or CPU tensor are checked; a device tensor is not read (the sampler ignores the bits above 11).  `tracks` holds
    names from TRACK_NAMES or indices 0..3, `empty` is "free" or "rest"; `B` and `n_bars`, when given, are what the sets must
    fit.  Returns (sets as an integer tensor on the device it came from, track_bits)."""
    if empty not in ("free", "rest"):
        raise ValueError(f"empty must be 'free' or 'rest', got {empty!r}")
    if isinstance(tracks, (str, bytes)) or not isinstance(tracks, (list, tuple, set, frozenset)):
        raise ValueError(f"tracks must be a list of names from {TRACK_NAMES} or indices 0..3, got {tracks!r}")
    track_bits = 0
    for k in tracks:
        if isinstance(k, str) and k in TRACK_NAMES:
            k = TRACK_NAMES.index(k)
        if not (_integer(k) and 0 <= k < 4):
            raise ValueError(f"tracks must hold names from {TRACK_NAMES} or indices 0..3, got {k!r}")
        track_bits |= 1 << int(k)
    if isinstance(sets, torch.Tensor):
        t = sets
        if t.dtype not in (torch.uint8, torch.int8, torch.int16, I32, I64):
            raise ValueError(f"sets must hold integers, got {t.dtype}")
    else:
        try:
            a = np.asarray(sets)
        except Exception as e:
            raise ValueError(f"sets must be an int tensor or array-like, got {type(sets).__name__}") from e
        if a.dtype.kind not in "iu":
            raise ValueError(f"sets must hold integers, got {a.dtype}")
        if a.size and (int(a.min()) < 0 or int(a.max()) >= 4096):            # (before the cast can wrap)
            raise ValueError(f"sets must hold values in [0, 4096), got {int(a.min())} .. {int(a.max())}")
        t = torch.from_numpy(np.ascontiguousarray(a.astype(np.int64)))
    if t.dim() not in (2, 3) or 0 in t.shape or t.shape[-1] not in SEG_STEPS:
        raise ValueError(f"sets must be [n_bars,S] or [B,n_bars,S] with S in {SEG_STEPS}, got {tuple(t.shape)}")
    if not t.is_cuda and (int(t.min()) < 0 or int(t.max()) >= 4096):
        raise ValueError(f"sets must hold values in [0, 4096), got {int(t.min())} .. {int(t.max())}")
    if n_bars is not None and t.shape[-2] != n_bars:
        raise ValueError(f"harmony: sets hold {t.shape[-2]} bars, the call has n_bars = {n_bars}")
    if B is not None and t.dim() == 3 and t.shape[0] != B:
        raise ValueError(f"harmony: sets hold {t.shape[0]} pieces, the call has B = {B}")
    return t, track_bits


def sample_chords_at(c_logits: torch.Tensor, node_cell: torch.Tensor, chart: torch.Tensor, track_bits: int = 0b1110,
                     temperature=1.0, top_k: Optional[int] = None, top_p: Optional[float] = None, seed: int = 0, min_notes=1,
                     max_notes=14, allowed_pitches=None):
    """`pm_sample_chords_at` ("Harmony" in include/polyphemus_hip.h): `sample_chords` under a chart of pitch-class sets.
    `node_cell` is int32 [N] (see `node_cells`: the track, bar and step of every node), `chart` int32 [G,32] on the device of
    `c_logits`: bits 0..11 of chart[g][t] are the pitch classes that may be drawn at step t of bar g by the tracks whose bit
    is set in `track_bits` (bit k = track k; the default binds Bass, Guitar and Strings).  A pitch of a bound track must be
    allowed by `allowed_pitches` and by its cell's set; a set that leaves none gives an empty chord, whatever `min_notes`
    says.  Everything else, the noise stream included, is `sample_chords`: with `track_bits` 0 or every set 0xfff the result
    is its result bit for bit.  Returns (tokens int32 [N,15,2], note_count int32 [N])."""
    from ._lib import PmChordRules
    _chk(c_logits, F32, "c_logits")
    if c_logits.dim() != 3 or c_logits.shape[1:] != (C.MAX_SIMU_TOKENS - 1, C.D_TOKEN_PAIR):
        raise ValueError("c_logits must be [N,15,230]")
    temps, mn, mx, words = check_chord_args(temperature, top_k, top_p, seed, min_notes, max_notes, allowed_pitches)
    N = c_logits.shape[0]
    if not isinstance(node_cell, torch.Tensor) or node_cell.dtype != I32 or node_cell.dim() != 1 or not node_cell.is_contiguous():
        raise ValueError("node_cell must be a contiguous int32 tensor [N]")
    if node_cell.shape[0] != N or node_cell.device != c_logits.device:
        raise ValueError(f"node_cell must be int32 [N = {N}] on {c_logits.device}, got [{node_cell.shape[0]}] on {node_cell.device}")
    if (not isinstance(chart, torch.Tensor) or chart.dtype != I32 or chart.dim() != 2 or chart.shape[0] < 1 or chart.shape[1] != 32
            or not chart.is_contiguous()):
        raise ValueError("chart must be a contiguous int32 tensor [G,32] with G >= 1")
    if chart.device != c_logits.device:
        raise ValueError(f"chart lives on {chart.device}, c_logits on {c_logits.device}")
    if not (_integer(track_bits) and 0 <= track_bits <= 15):
        raise ValueError(f"track_bits must be an int in [0, 15], got {track_bits!r}")
    tokens = torch.empty(N, C.MAX_SIMU_TOKENS - 1, 2, dtype=I32, device=c_logits.device)
    note_count = torch.empty(N, dtype=I32, device=c_logits.device)
    if N:
        rules = PmChordRules()
        rules.temperature[0], rules.temperature[1] = temps
        rules.top_k = 0 if top_k is None else min(int(top_k), 1 << 30)
        rules.top_p = 1.0 if top_p is None else float(top_p)
        for k in range(4):
            rules.min_notes[k], rules.max_notes[k] = mn[k], mx[k]
            for w in range(4):
                rules.pitch_mask[k][w] = words[k][w]
        call("pm_sample_chords_at", ptr(c_logits), ptr(node_cell), N, ptr(chart), chart.shape[0], int(track_bits),
             ctypes.addressof(rules), int(seed), ptr(tokens), ptr(note_count), stream())
    return tokens, note_count


def check_structure_args(temperature=1.0, threshold=0.5, min_active=0, max_active=32, allowed_steps=None, seed=None):
    """The argument rules of structure sampling (`sample_structure`, `generate.generate_music(structure_rules=...)`): raises
    ValueError naming the argument, before anything touches the device.  `temperature` is a finite number >= 0; `threshold`
    a number or four numbers (Drums, Bass, Guitar, Strings) in (0, 1); `min_active` / `max_active` an int or four ints with
    0 <= min_active <= max_active <= 32 and min_active no larger than the track's allowed steps; `allowed_steps` None or a
    bool array-like [4,32]; some track must keep max_active > 0 and an allowed step.
    Returns (temperature, bias [4] = logit(threshold) in double, min_active [4], max_active [4], step_mask: 4 words of 32 bits)."""
    if not (_real(temperature) and math.isfinite(temperature) and temperature >= 0):
        raise ValueError(f"temperature must be a finite number >= 0, got {temperature!r}")
    check_sampling_args(None, None, None, seed)
    th = tuple(threshold) if isinstance(threshold, (tuple, list, np.ndarray)) else (threshold,) * 4
    if len(th) != 4 or not all(_real(v) and 0 < v < 1 for v in th):
        raise ValueError(f"threshold must be a number or four numbers (one per track) in (0, 1), got {threshold!r}")
    bias = tuple(math.log(float(v) / (1.0 - float(v))) for v in th)          # (finite in fp32 for every double in (0, 1))

    mx = _four(max_active, "max_active")
    if not all(0 <= a <= 32 for a in mx):
        raise ValueError(f"max_active must be in [0, 32], got {max_active!r}")
    mn = _four(min_active, "min_active")
    if not all(0 <= a <= b for a, b in zip(mn, mx)):
        raise ValueError(f"min_active must satisfy 0 <= min_active <= max_active = {max_active!r}, got {min_active!r}")
    words = [row[0] for row in _mask_words(allowed_steps, (4, 32), "allowed_steps")]
    steps = [bin(w).count("1") for w in words]
    if not all(a <= n for a, n in zip(mn, steps)):
        raise ValueError(f"min_active must not exceed the allowed steps of its track ({steps} in allowed_steps), got {min_active!r}")
    if not any(b > 0 and n > 0 for b, n in zip(mx, steps)):
        raise ValueError(f"no track is left with max_active > 0 and an allowed step: max_active = {max_active!r}, "
                         f"allowed_steps leaves {steps} steps")
    return float(temperature), bias, mn, mx, words


def sample_structure(s_logits: torch.Tensor, temperature: float = 1.0, threshold=0.5, min_active=0, max_active=32,
                     allowed_steps=None, seed: int = 0, return_counts: bool = False):
    """`pm_sample_structure` ("Structure sampling" in include/polyphemus_hip.h): the active cells of every bar of `s_logits`
    ([...,4,32] fp32) drawn from the model's probabilities, a cell on with probability sigmoid((x - logit(threshold)) /
    temperature) where no bound binds (temperature 0 = the thresholded structure), each track keeping between `min_active`
    and `max_active` cells on the steps `allowed_steps` ([4,32] bool, None = all) gives it, and no bar left empty.  The bars
    are numbered along the flattened leading dimensions; a pure function of the logits, the rules and `seed`.  Returns a
    bool tensor of s_logits' shape, and with `return_counts` the int32 [...,4] active cells per (bar, track)."""
    from ._lib import PmStructureRules
    T, bias, mn, mx, words = check_structure_args(temperature, threshold, min_active, max_active, allowed_steps, seed)
    _chk(s_logits, F32, "s_logits")
    if s_logits.dim() < 2 or s_logits.shape[-2:] != (4, 32):
        raise ValueError("s_logits must be [..., 4, 32]")
    G, dev = s_logits.numel() // 128, s_logits.device
    if G >= 1 << 31:
        raise ValueError(f"s_logits holds {G} bars, the kernel takes fewer than 2^31")
    out = torch.empty(s_logits.shape, dtype=U8, device=dev)
    counts = torch.empty(*s_logits.shape[:-2], 4, dtype=I32, device=dev) if return_counts else None
    if G:
        rules = PmStructureRules()
        rules.temperature = T
        for k in range(4):
            rules.bias[k], rules.min_active[k], rules.max_active[k], rules.step_mask[k] = bias[k], mn[k], mx[k], words[k]
        call("pm_sample_structure", ptr(s_logits), G, ctypes.addressof(rules), int(seed), None, ptr(out), ptr(counts), stream())
    return (out.view(torch.bool), counts) if return_counts else out.view(torch.bool)


def gcl_forward_fused(x, T, plan: Plan, dropout_p: float, seed: int, layer_uid: int, w_frag, bias, col_stats=None,
                      planes=None, use_classes: bool = True):
    """`pm_gcl_forward_fused`: h = A'(x) @ [W_t; W_4; W_5; root] + bias of one GCL layer in one kernel (compact graphs,
    d in {128, 256, 512}); `w_frag` = `split_planes_frag(W, 1)`; `planes` (int16 [3, N*4d], optional) receives the A' planes."""
    _chk(x, F32, "x"); _chk(T, F32, "T")
    N, d = x.shape
    h = torch.empty(N, d, dtype=F32, device=x.device)
    call("pm_gcl_forward_fused", ptr(x), ptr(T), ptr(plan.buf), N, plan.E, plan.G, d, float(dropout_p),
         seed & 0xFFFFFFFF, layer_uid, ptr(w_frag), ptr(bias), 1 if use_classes else 0, ptr(h), ptr(col_stats),
         ptr(planes), 0 if planes is None else planes.shape[1], stream())
    return h


def gcl_forward_fused_sel(x, T, plan: Plan, dropout_p: float, seed: int, layer_uid: int, w_frag, bias, col_stats=None,
                          planes=None, use_classes: bool = True, self_planes: bool = False, h2=None):
    """`pm_gcl_forward_fused_sel` / `_sel_h2` (with `h2`, the address of a PmH2): `gcl_forward_fused` that leaves columns
    [3d, 4d) of `planes` (the self block: the split of x itself) unwritten unless `self_planes`."""
    _chk(x, F32, "x"); _chk(T, F32, "T")
    N, d = x.shape
    h = torch.empty(N, d, dtype=F32, device=x.device)
    head = (ptr(x), ptr(T), ptr(plan.buf), N, plan.E, plan.G, d, float(dropout_p), seed & 0xFFFFFFFF, layer_uid, ptr(w_frag),
            ptr(bias), 1 if use_classes else 0, ptr(h), ptr(col_stats), ptr(planes), 0 if planes is None else planes.shape[1])
    if h2 is None:
        call("pm_gcl_forward_fused_sel", *head, 1 if self_planes else 0, stream())
    else:
        call("pm_gcl_forward_fused_sel_h2", *head, h2, 1 if self_planes else 0, stream())
    return h


def gcl_forward_from_planes(a_planes, plan: Plan, d: int, w_frag, bias, col_stats=None, use_classes: bool = True):
    """`pm_gcl_forward_from_planes`: h = A' @ [W_t; W_4; W_5; root] + bias with the aggregate read from the planes
    `pm_segreduce_fwd_planes` wrote (int16 [3, N*4d]); the dense-graph path at d = 512."""
    N = plan.N
    h = torch.empty(N, d, dtype=F32, device=a_planes.device)
    call("pm_gcl_forward_from_planes", ptr(a_planes), a_planes.shape[1], ptr(plan.buf), N, plan.E, plan.G, d, ptr(w_frag),
         ptr(bias), 1 if use_classes else 0, ptr(h), ptr(col_stats), stream())
    return h


def gcl_input_grad_fused(dh_planes, plan: Plan, d: int, w_frag_t, use_classes: bool = True, out=None):
    """`pm_gcl_input_grad_fused`: dA' [N, 4d] = dh @ [W_t; W_4; W_5; root]^T per track group, A-stationary;
    `dh_planes` int16 [3, N*d] (`split_planes(dh)`), `w_frag_t` = `split_planes_frag(W, 0)`."""
    N = plan.N
    dA = out if out is not None else torch.empty(N, 4 * d, dtype=F32, device=dh_planes.device)
    call("pm_gcl_input_grad_fused", ptr(dh_planes), dh_planes.shape[1], ptr(plan.buf), N, plan.E, plan.G, d, ptr(w_frag_t),
         1 if use_classes else 0, ptr(dA), stream())
    return dA


class _BnBwd(ctypes.Structure):          # PmBnBwd (include/polyphemus_hip.h)
    _fields_ = [(k, ctypes.c_void_p) for k in ("h", "du", "mean", "var", "gamma", "beta", "acc3", "dgamma", "dbeta", "dbias_pre")] + \
               [("eps", ctypes.c_float), ("relu", ctypes.c_int32), ("add_residual", ctypes.c_int32), ("reserved", ctypes.c_int32)]


def bn_bwd_sums(h, du, mean, var, gamma, beta, eps: float = 1e-5, relu: bool = True):
    """`pm_bn_bwd_sums`: the three column sums of the norm backward, fp64 [PM_BN_REPL, 3, C]."""
    O, Cc = h.shape
    acc3 = torch.zeros(8, 3, Cc, dtype=torch.float64, device=h.device)
    call("pm_bn_bwd_sums", ptr(h), ptr(du), O, Cc, ptr(mean), ptr(var), float(eps), ptr(gamma), ptr(beta), 1 if relu else 0,
         ptr(acc3), stream())
    return acc3


def gcl_input_grad_bn(h, du, mean, var, gamma, beta, acc3, plan: Plan, w_frag_t, dgamma=None, dbeta=None, dbias_pre=None,
                      eps: float = 1e-5, relu: bool = True, use_classes: bool = True, add_residual: bool = False):
    """`pm_gcl_input_grad_bn`: the norm backward inside the input gradient; returns (dA' [N, 4d], dh planes int16 [3, N*d])."""
    N, d = h.shape
    dA = torch.empty(N, 4 * d, dtype=F32, device=h.device)
    planes = torch.empty(3, N * d, dtype=torch.int16, device=h.device)
    nb = _BnBwd(ptr(h), ptr(du), ptr(mean), ptr(var), ptr(gamma), ptr(beta), ptr(acc3), ptr(dgamma), ptr(dbeta), ptr(dbias_pre),
                float(eps), 1 if relu else 0, 1 if add_residual else 0, 0)
    call("pm_gcl_input_grad_bn", ctypes.addressof(nb), ptr(planes), planes.shape[1], ptr(plan.buf), N, plan.E, plan.G, d,
         ptr(w_frag_t), 1 if use_classes else 0, ptr(dA), stream())
    return dA, planes


def gcl_weight_grad_fused(a_planes, dh_planes, plan: Plan, d: int, dW, use_classes: bool = True):
    """`pm_gcl_weight_grad_fused`: dW [7d, d] += A'^T dh per track group (stacked [W_t; W_4; W_5; root] rows);
    `a_planes` int16 [3, N*4d], `dh_planes` int16 [3, N*d]."""
    _chk(dW, F32, "dW")
    call("pm_gcl_weight_grad_fused", ptr(a_planes), a_planes.shape[1], ptr(dh_planes), dh_planes.shape[1], ptr(plan.buf),
         plan.N, plan.E, plan.G, d, 1 if use_classes else 0, ptr(dW), stream())
    return dW


def gcl_weight_grad_fused_x(a_planes, x, dh_planes, plan: Plan, d: int, dW, use_classes: bool = True, a_scale=None, dh_scale=None):
    """`pm_gcl_weight_grad_fused_x` / `_x_h2` (with the two device scales of the pair format): `gcl_weight_grad_fused` whose
    self-block tiles read the rows of `x` [N, d] (the forward's input) instead of columns [3d, 4d) of `a_planes`."""
    _chk(dW, F32, "dW"); _chk(x, F32, "x")
    head = (ptr(a_planes), a_planes.shape[1], ptr(x), ptr(dh_planes), dh_planes.shape[1], ptr(plan.buf), plan.N, plan.E, plan.G, d,
            1 if use_classes else 0, ptr(dW))
    if a_scale is None:
        call("pm_gcl_weight_grad_fused_x", *head, stream())
    else:
        call("pm_gcl_weight_grad_fused_x_h2", *head, ptr(a_scale), ptr(dh_scale), stream())
    return dW


def segreduce_fwd(x, T, plan: Plan, dropout_p: float, seed: int, layer_uid: int, out=None):
    _chk(x, F32, "x"); _chk(T, F32, "T")
    N, d = x.shape
    A = out if out is not None else torch.empty(N, 7 * d, dtype=F32, device=x.device)
    e0 = _prof_begin("segreduce_fwd")
    call("pm_segreduce_fwd", ptr(x), ptr(T), ptr(plan.buf), N, plan.E, plan.G, d, float(dropout_p),
         seed & 0xFFFFFFFF, layer_uid, 0, ptr(A), stream())
    _prof_end("segreduce_fwd", e0, 4.0 * d * N * (1 + C.N_EDGE_TYPES) + 12.0 * plan.E)   # algorithmic HBM bytes
    return A


def segreduce_bwd(x, T, dA, dres, plan: Plan, dropout_p: float, seed: int, layer_uid: int, dT, out=None):
    _chk(x, F32, "x"); _chk(dA, F32, "dA"); _chk(dres, F32, "dres", allow_none=True); _chk(dT, F32, "dT")
    N, d = x.shape
    dx = out if out is not None else torch.empty(N, d, dtype=F32, device=x.device)
    call("pm_segreduce_bwd", ptr(x), ptr(T), ptr(dA), ptr(dres), ptr(plan.buf), N, plan.E, plan.G, d,
         float(dropout_p), seed & 0xFFFFFFFF, layer_uid, 0, ptr(dx), ptr(dT), stream())
    return dx


GEMM_RELU, GEMM_ACCUM, GEMM_PARTITION, GEMM_RELU_ADD = 1, 2, 4, 16


def bn_fold_weights(W, bias, gamma, beta, running_mean, running_var, eps=1e-5):
    """(W * s, bias * s + t) with s = gamma / sqrt(running_var + eps), t = beta - running_mean * s (columns of W)."""
    W2 = W.reshape(-1, W.shape[-1])
    Wo, bo = torch.empty_like(W2), torch.empty_like(bias)
    call("pm_bn_fold_weights", ptr(W2), W2.shape[0], W2.shape[1], ptr(bias), ptr(gamma), ptr(beta), ptr(running_mean),
         ptr(running_var), eps, ptr(Wo), ptr(bo), stream())
    return Wo, bo


def gemm(A, B, out, M, N, K, lda, ldb, ldc, transA=False, transB=False, bias=None, relu=False, accum=False,
         split_k=1, rowmap=None, rows_per_entry=0, dyn_entries=None, relu_add=False):
    """out[M,N] (=|+=) op(A) op(B) (+bias)(relu); A/B/out may be views with an element offset
    (pass the sliced tensor: its data_ptr() carries the offset) and explicit leading dimensions.
    relu_add: out = out + relu(op(A) op(B) + bias)."""
    flags = (GEMM_RELU if relu else 0) | (GEMM_ACCUM if accum else 0) | (GEMM_RELU_ADD if relu_add else 0)
    cls = gemm_class(transA, transB, M, N, K) if PROF is not None else ""
    e0 = _prof_begin(cls)
    call("pm_gemm_f32", int(transA), int(transB), M, N, K, ptr(A), lda, ptr(B), ldb, ptr(out), ldc, ptr(bias),
         flags, split_k, ptr(rowmap), rows_per_entry, ptr(dyn_entries), stream())
    _prof_end(cls, e0, 2.0 * M * N * K)                                                  # algorithmic flops
    return out


class _GemmDesc(ctypes.Structure):
    """ctypes mirror of PmGemmDesc (include/polyphemus_hip.h)."""
    _fields_ = [("transA", ctypes.c_int32), ("transB", ctypes.c_int32), ("M", ctypes.c_int32), ("N", ctypes.c_int32),
                ("K", ctypes.c_int32), ("A", ctypes.c_void_p), ("lda", ctypes.c_int32), ("B", ctypes.c_void_p),
                ("ldb", ctypes.c_int32), ("C", ctypes.c_void_p), ("ldc", ctypes.c_int32), ("bias", ctypes.c_void_p),
                ("flags", ctypes.c_int32), ("split_k", ctypes.c_int32), ("rowmap", ctypes.c_void_p),
                ("rows_per_entry", ctypes.c_int32), ("dyn_entries", ctypes.c_void_p), ("n_groups", ctypes.c_int32),
                ("a_group_stride", ctypes.c_int64), ("b_group_stride", ctypes.c_int64),
                ("c_group_stride", ctypes.c_int64), ("bias_group_stride", ctypes.c_int64),
                ("map_group_stride", ctypes.c_int32), ("dyn_group_stride", ctypes.c_int32),
                ("b_split_rows", ctypes.c_int32), ("b_shared_off", ctypes.c_int64),
                ("c_split_rows", ctypes.c_int32), ("c_shared_off", ctypes.c_int64), ("col_stats", ctypes.c_void_p),
                ("operand_planes", ctypes.c_int32), ("a_plane_stride", ctypes.c_int64),
                ("b_plane_stride", ctypes.c_int64), ("class_ptr", ctypes.c_void_p), ("class_block", ctypes.c_int32),
                ("b_frag", ctypes.c_void_p), ("a_colsum", ctypes.c_void_p)]


def gemm_desc(A, B, out, M, N, K, lda, ldb, ldc, transA=False, transB=False, bias=None, relu=False, accum=False,
              split_k=1, rowmap=None, rows_per_entry=0, dyn_entries=None, n_groups=1, a_group_stride=0,
              b_group_stride=0, c_group_stride=0, bias_group_stride=0, map_group_stride=0, dyn_group_stride=0,
              b_split_rows=0, b_shared_off=0, c_split_rows=0, c_shared_off=0, partition=False, col_stats=None, planes=False, a_plane_stride=0,
              b_plane_stride=0, class_ptr=None, class_block=0, b_frag=None, a_colsum=None):
    """Grouped / stacked-operand GEMM (`pm_gemm_f32_desc`): see PmGemmDesc in the header."""
    q = _GemmDesc(int(transA), int(transB), M, N, K, ptr(A), lda, ptr(B), ldb, ptr(out), ldc, ptr(bias),
                  (GEMM_RELU if relu else 0) | (GEMM_ACCUM if accum else 0) | (GEMM_PARTITION if partition else 0),
                  split_k, ptr(rowmap), rows_per_entry,
                  ptr(dyn_entries), n_groups, a_group_stride, b_group_stride, c_group_stride, bias_group_stride,
                  map_group_stride, dyn_group_stride, b_split_rows, b_shared_off, c_split_rows, c_shared_off, ptr(col_stats), int(planes), a_plane_stride, b_plane_stride, ptr(class_ptr), class_block,
                  ptr(b_frag), ptr(a_colsum))
    call("pm_gemm_f32_desc", ctypes.addressof(q), stream())
    return out


def split_planes(x: torch.Tensor) -> torch.Tensor:
    """fp32 tensor -> int16 [3, numel] holding the three bf16 planes with x = p1 + p2 + p3 exactly
    (`pm_split_planes`; the operand format of `gemm_desc(..., planes=True)`)."""
    _chk(x, F32, "x")
    n = x.numel()
    out = torch.empty(3, n, dtype=torch.int16, device=x.device)
    call("pm_split_planes", ptr(x), n, ptr(out), n, stream())
    return out


def split_planes_frag(W: torch.Tensor, kind: int) -> torch.Tensor:
    """Fragment-major bf16 planes of weight matrices W [n_mats, rows, cols] or [rows, cols] (`pm_split_planes_frag`;
    the `b_frag` operand of `gemm_desc`): kind 0 for a product that uses W transposed (transB), 1 otherwise."""
    _chk(W, F32, "W")
    mats = W.shape[0] if W.dim() == 3 else 1
    rows, cols = W.shape[-2:]
    out = torch.empty(mats, rows * cols * 3, dtype=torch.int16, device=W.device)
    call("pm_split_planes_frag", ptr(W), rows, cols, kind, mats, rows * cols, rows * cols * 3, ptr(out), stream())
    return out


def linear(x, weight, bias=None, relu=False, out=None):
    """y = x @ weight.T + bias for contiguous x [M,K], weight [N,K] (nn.Linear layout)."""
    M, K = x.shape
    N = weight.shape[0]
    y = out if out is not None else torch.empty(M, N, dtype=F32, device=x.device)
    return gemm(x, weight, y, M, N, K, x.stride(0), weight.stride(0), y.stride(0), transB=True, bias=bias, relu=relu)


def bn_scratch(C_: int, device) -> torch.Tensor:
    return torch.empty(256 * 3 * C_ + 4 * C_, dtype=F64, device=device)          # PM_BN_SCRATCH(C)


def bn_stats(x, O, C_, I, running_mean=None, running_var=None, momentum=0.1, scratch=None):
    mean = torch.empty(C_, dtype=F32, device=x.device)
    var = torch.empty(C_, dtype=F32, device=x.device)
    scratch = scratch if scratch is not None else bn_scratch(C_, x.device)
    call("pm_bn_stats", ptr(x), O, C_, I, ptr(mean), ptr(var), ptr(running_mean), ptr(running_var), momentum,
         ptr(scratch), stream())
    return mean, var


def bn_apply(x, O, C_, I, mean, var, gamma, beta, eps=1e-5, residual=None, relu=False, out=None):
    y = out if out is not None else torch.empty_like(x)
    call("pm_bn_apply", ptr(x), O, C_, I, ptr(mean), ptr(var), eps, ptr(gamma), ptr(beta), ptr(residual), int(relu),
         ptr(y), stream())
    return y


def bn_bwd(x, dy, O, C_, I, mean, var, gamma, beta, dgamma, dbeta, eps=1e-5, relu=False, out=None, scratch=None,
           dbias_pre=None):
    dx = out if out is not None else torch.empty_like(x)
    scratch = scratch if scratch is not None else bn_scratch(C_, x.device)
    call("pm_bn_bwd", ptr(x), ptr(dy), O, C_, I, ptr(mean), ptr(var), eps, ptr(gamma), ptr(beta), int(relu),
         ptr(dgamma), ptr(dbeta), ptr(dbias_pre), ptr(dx), ptr(scratch), stream())
    return dx


# ---- split forms for synchronised BatchNorm (data parallel, statistics over the global batch) -----------------------------
def bn_partial_sums(x, O, C_, I, dy=None, mean=None, var=None, gamma=None, beta=None, eps=1e-5, relu=False):
    """[3][C] fp64 column sums of this rank: {sum x, sum x^2, 0}, or with dy {sum du, sum du*xhat, sum xhat}."""
    sums = torch.empty(3, C_, dtype=F64, device=x.device)
    call("pm_bn_partial_sums", ptr(x), ptr(dy), O, C_, I, ptr(mean), ptr(var), eps, ptr(gamma), ptr(beta), int(relu),
         ptr(sums), ptr(bn_scratch(C_, x.device)), stream())
    return sums


def bn_stats_from_sums(sums, count, C_, running_mean=None, running_var=None, momentum=0.1):
    mean = torch.empty(C_, dtype=F32, device=sums.device)
    var = torch.empty(C_, dtype=F32, device=sums.device)
    call("pm_bn_stats_from_sums", ptr(sums), float(count), C_, ptr(mean), ptr(var), ptr(running_mean), ptr(running_var),
         momentum, stream())
    return mean, var


def bn_bwd_from_sums(x, dy, O, C_, I, mean, var, gamma, beta, sums_local, sums_global, count_global, dgamma, dbeta, eps=1e-5,
                     relu=False, dbias_pre=None):
    dx = torch.empty_like(x)
    scratch = torch.empty(2 * C_, dtype=F64, device=x.device)
    call("pm_bn_bwd_from_sums", ptr(x), ptr(dy), O, C_, I, ptr(mean), ptr(var), eps, ptr(gamma), ptr(beta), int(relu),
         ptr(sums_local), ptr(sums_global), float(count_global), ptr(dgamma), ptr(dbeta), ptr(dbias_pre), ptr(dx),
         ptr(scratch), stream())
    return dx


def relu_bwd(dy, y, out=None):
    dx = out if out is not None else torch.empty_like(dy)
    call("pm_relu_bwd", ptr(dy), ptr(y), dy.numel(), ptr(dx), stream())
    return dx


def relu_residual(x, res=None):
    y = torch.empty_like(x)
    call("pm_relu_residual_fwd", ptr(x), ptr(res), x.numel(), ptr(y), stream())
    return y


def dropout_rows(x, cols: int, p: float, seed: int, site: int, out=None):
    """x viewed as [numel / cols, cols] times the counter-hash keep mask of (seed, site) / (1 - p); contiguous input."""
    if not x.is_contiguous():
        raise ValueError("dropout_rows needs a contiguous tensor")
    y = out if out is not None else torch.empty_like(x)
    call("pm_dropout_rows", ptr(x), x.numel() // cols, cols, float(p), seed & 0xFFFFFFFF, site, ptr(y), stream())
    return y


def add(a, b, out=None):
    o = out if out is not None else torch.empty_like(a)
    call("pm_add", ptr(a), ptr(b), a.numel(), ptr(o), stream())
    return o


def grad_accumulate(grads, accum, scale: float, first: bool):
    """accum = (0 if first else accum) + scale * grads (training.py:149,158)."""
    _chk(grads, F32, "grads"); _chk(accum, F32, "accum")
    if grads.numel() != accum.numel():
        raise ValueError("grads / accum size mismatch")
    call("pm_grad_accumulate", ptr(grads), ptr(accum), grads.numel(), float(scale), int(bool(first)), stream())
    return accum


def colsum_acc(x, M, C_, ld, out):
    call("pm_colsum_acc", ptr(x), M, C_, ld, ptr(out), stream())


def colsum_rows_acc(x, C_, ld, rowmap, rows_per_entry, dyn_entries, max_entries, out):
    call("pm_colsum_rows_acc", ptr(x), C_, ld, ptr(rowmap), rows_per_entry, ptr(dyn_entries), max_entries, ptr(out),
         stream())


def reparam_fwd(mu, log_var, eps):
    z = torch.empty_like(mu)
    call("pm_reparam_fwd", ptr(mu), ptr(log_var), ptr(eps), mu.numel(), ptr(z), stream())
    return z


def reparam_bwd(dz, log_var, eps, dmu, dlog_var):
    call("pm_reparam_bwd", ptr(dz), ptr(log_var), ptr(eps), dz.numel(), ptr(dmu), ptr(dlog_var), stream())


def gate_fwd(x, w, b):
    N, d = x.shape
    g = torch.empty(N, dtype=F32, device=x.device)
    call("pm_gate_fwd", ptr(x), ptr(w), ptr(b), N, d, ptr(g), stream())
    return g


def attnpool_fwd(x, g, g_mean, g_var, bn_g, bn_b, plan: Plan, eps=1e-5):
    N, d = x.shape
    alpha = torch.empty(N, dtype=F32, device=x.device)
    out = torch.empty(plan.G, d, dtype=F32, device=x.device)
    call("pm_attnpool_fwd", ptr(x), ptr(g), ptr(g_mean), ptr(g_var), eps, ptr(bn_g), ptr(bn_b), ptr(plan.buf), N,
         plan.E, plan.G, d, ptr(alpha), ptr(out), stream())
    return alpha, out


def attnpool_bwd(x, g, g_mean, g_var, bn_g, alpha, dout, gate_w, plan: Plan, d_gate_w, d_gate_b, d_bn_g, d_bn_b,
                 eps=1e-5, x_gate=None):
    """Returns dx, or (dx, dx_gate) when the gate MLP saw `x_gate` instead of x (dropout in front of its Linear)."""
    N, d = x.shape
    dx = torch.empty_like(x)
    dxg = torch.empty_like(x) if x_gate is not None else None
    scratch = torch.empty(3 * N + 8, dtype=F32, device=x.device)
    call("pm_attnpool_bwd", ptr(x), ptr(g), ptr(g_mean), ptr(g_var), eps, ptr(bn_g), ptr(alpha), ptr(dout),
         ptr(gate_w), ptr(plan.buf), N, plan.E, plan.G, d, ptr(dx), ptr(d_gate_w), ptr(d_gate_b), ptr(d_bn_g),
         ptr(d_bn_b), ptr(scratch), ptr(x_gate), ptr(dxg), stream())
    return dx if x_gate is None else (dx, dxg)


def attnpool_bwd_sync(x, g, g_mean, g_var, bn_g, alpha, dout, gate_w, plan: Plan, d_gate_w, d_gate_b, d_bn_g, d_bn_b, reduce_,
                      count_global, eps=1e-5, x_gate=None):
    """`attnpool_bwd` with the BatchNorm1d(1) of the gate synchronised over the ranks: `reduce_(t)` sums a tensor in place
    over the ranks, `count_global` is the global node count."""
    N, d = x.shape
    dx = torch.empty_like(x)
    dxg = torch.empty_like(x) if x_gate is not None else None
    scratch = torch.empty(3 * N + 8, dtype=F32, device=x.device)
    call("pm_attnpool_bwd_sums", ptr(x), ptr(g), ptr(g_mean), ptr(g_var), eps, ptr(alpha), ptr(dout), ptr(plan.buf), N,
         plan.E, plan.G, d, ptr(scratch), stream())
    gs = scratch[:4].view(F64).clone()                     # the two local sums (fp64 at the head of the scratch)
    reduce_(gs)
    call("pm_attnpool_bwd_from_sums", ptr(x), ptr(g), ptr(g_mean), ptr(g_var), eps, ptr(bn_g), ptr(alpha), ptr(dout),
         ptr(gate_w), ptr(plan.buf), N, plan.E, plan.G, d, ptr(dx), ptr(d_gate_w), ptr(d_gate_b), ptr(d_bn_g), ptr(d_bn_b),
         ptr(scratch), ptr(x_gate), ptr(dxg), ptr(gs), float(count_global), stream())
    return dx if x_gate is None else (dx, dxg)


def bar_broadcast_fwd(bars, plan: Plan):
    d = bars.shape[1]
    x = torch.empty(plan.N, d, dtype=F32, device=bars.device)
    call("pm_bar_broadcast_fwd", ptr(bars), ptr(plan.buf), plan.N, plan.E, plan.G, d, ptr(x), stream())
    return x


def bar_broadcast_bwd(dx, plan: Plan):
    d = dx.shape[1]
    db = torch.empty(plan.G, d, dtype=F32, device=dx.device)
    call("pm_bar_broadcast_bwd", ptr(dx), ptr(plan.buf), plan.N, plan.E, plan.G, d, ptr(db), stream())
    return db


def conv3x3_fwd(x, w, b, G, Ci, Co, H, W, up4=False):
    y = torch.empty(G, Co, H, W, dtype=F32, device=x.device)
    call("pm_conv3x3_fwd", ptr(x), ptr(w), ptr(b), G, Ci, Co, H, W, int(up4), ptr(y), stream())
    return y


def conv3x3_bwd_data(dy, w, G, Ci, Co, H, W, up4=False):
    dx = torch.empty(G, Ci, H, W // 4 if up4 else W, dtype=F32, device=dy.device)
    call("pm_conv3x3_bwd_data", ptr(dy), ptr(w), G, Ci, Co, H, W, int(up4), ptr(dx), stream())
    return dx


def conv3x3_bwd_weight(x, dy, G, Ci, Co, H, W, dw, db, up4=False):
    call("pm_conv3x3_bwd_weight", ptr(x), ptr(dy), G, Ci, Co, H, W, int(up4), ptr(dw), ptr(db), stream())


def maxpool4_fwd(x):
    y = torch.empty(*x.shape[:-1], x.shape[-1] // 4, dtype=F32, device=x.device)
    call("pm_maxpool4_fwd", ptr(x), y.numel(), ptr(y), stream())
    return y


def maxpool4_bwd(x, dy):
    dx = torch.empty_like(x)
    call("pm_maxpool4_bwd", ptr(x), ptr(dy), dy.numel(), ptr(dx), stream())
    return dx


# ---- the training step's CNN chains as bar-resident kernels (model.py:219-230 / 279-285 with BatchNorm2d on batch statistics) ----
def cnn_enc_fwd(s, w0, b0, gamma1, beta1, w4, b4, gamma5, beta5, G, rmean1=None, rvar1=None, rmean5=None, rvar5=None,
                eps=1e-5, momentum=0.1, scratch=None):
    """conv0, BN1, ReLU, pool (1,4), conv4, BN5, ReLU over s [G,1,4,32]: dict of c0, a0, p0, c1, a1 and the saved mean / var
    of the two norms (m0, v0, m1, v1); the running statistics are updated in place."""
    dev = s.device
    o = {"c0": torch.empty(G, 8, 4, 32, dtype=F32, device=dev), "a0": torch.empty(G, 8, 4, 32, dtype=F32, device=dev),
         "p0": torch.empty(G, 8, 4, 8, dtype=F32, device=dev), "c1": torch.empty(G, 16, 4, 8, dtype=F32, device=dev),
         "a1": torch.empty(G, 16, 4, 8, dtype=F32, device=dev), "m0": torch.empty(8, dtype=F32, device=dev),
         "v0": torch.empty(8, dtype=F32, device=dev), "m1": torch.empty(16, dtype=F32, device=dev),
         "v1": torch.empty(16, dtype=F32, device=dev)}
    scratch = scratch if scratch is not None else bn_scratch(512, dev)      # (the step's at d = 256)
    call("pm_cnn_enc_fwd", ptr(s), ptr(w0), ptr(b0), ptr(gamma1), ptr(beta1), ptr(w4), ptr(b4), ptr(gamma5), ptr(beta5), G, eps,
         momentum, ptr(o["c0"]), ptr(o["a0"]), ptr(o["p0"]), ptr(o["c1"]), ptr(o["a1"]), ptr(o["m0"]), ptr(o["v0"]), ptr(rmean1),
         ptr(rvar1), ptr(o["m1"]), ptr(o["v1"]), ptr(rmean5), ptr(rvar5), ptr(scratch), scratch.numel(), stream())
    return o


def cnn_dec_fwd(u2, w1, b1, gamma2, beta2, w4, b4, G, rmean2=None, rvar2=None, eps=1e-5, momentum=0.1, scratch=None):
    """upsample (1,4), conv1, BN2, ReLU, conv4 over u2 [G,16,4,8]: dict of c2, a2, s_logits and the norm's saved m2, v2."""
    dev = u2.device
    o = {"c2": torch.empty(G, 8, 4, 32, dtype=F32, device=dev), "a2": torch.empty(G, 8, 4, 32, dtype=F32, device=dev),
         "s_logits": torch.empty(G, 1, 4, 32, dtype=F32, device=dev), "m2": torch.empty(8, dtype=F32, device=dev),
         "v2": torch.empty(8, dtype=F32, device=dev)}
    scratch = scratch if scratch is not None else bn_scratch(512, dev)      # (the step's at d = 256)
    call("pm_cnn_dec_fwd", ptr(u2), ptr(w1), ptr(b1), ptr(gamma2), ptr(beta2), ptr(w4), ptr(b4), G, eps, momentum, ptr(o["c2"]),
         ptr(o["a2"]), ptr(o["s_logits"]), ptr(o["m2"]), ptr(o["v2"]), ptr(rmean2), ptr(rvar2), ptr(scratch), scratch.numel(),
         stream())
    return o


def cnn_enc_bwd(s, fwd, da1, gamma1, beta1, gamma5, beta5, w4, G, dw0, db0, dgamma1, dbeta1, dw4, db4, dgamma5, dbeta5,
                eps=1e-5, scratch=None):
    """Backward of cnn_enc_fwd (`fwd`: its dict) from da1 [G,16,4,8]: the eight gradients accumulate (+=); returns dc1, da0, dc0."""
    dev = s.device
    dc1 = torch.empty(G, 16, 4, 8, dtype=F32, device=dev)
    da0 = torch.empty(G, 8, 4, 32, dtype=F32, device=dev)
    dc0 = torch.empty(G, 8, 4, 32, dtype=F32, device=dev)
    scratch = scratch if scratch is not None else bn_scratch(512, dev)      # (the step's at d = 256)
    call("pm_cnn_enc_bwd", ptr(s), ptr(fwd["c0"]), ptr(fwd["a0"]), ptr(fwd["p0"]), ptr(fwd["c1"]), ptr(da1), ptr(fwd["m0"]),
         ptr(fwd["v0"]), ptr(gamma1), ptr(beta1), ptr(fwd["m1"]), ptr(fwd["v1"]), ptr(gamma5), ptr(beta5), ptr(w4), G, eps,
         ptr(dw0), ptr(db0), ptr(dgamma1), ptr(dbeta1), ptr(dw4), ptr(db4), ptr(dgamma5), ptr(dbeta5), ptr(dc1), ptr(da0), ptr(dc0),
         ptr(scratch), scratch.numel(), stream())
    return dc1, da0, dc0


def content_ce(c_logits, plan: Plan, grad_scale=1.0, want_grad=True, out=None, dbias=None):
    """dbias = (d_bias_pitch_drum [131], d_bias_pitch_non_drum [131], d_bias_dur [99]) accumulates the
    un-embedding bias gradients inside the same pass (needs want_grad)."""
    N = c_logits.shape[0]
    out = out if out is not None else torch.empty(4, dtype=F64, device=c_logits.device)
    dl = torch.empty_like(c_logits) if want_grad else None
    b = dbias if dbias is not None else (None, None, None)
    call("pm_content_ce", ptr(c_logits), ptr(plan.tokens), ptr(plan.tok_hist), ptr(plan.is_drum), N, C.N_SLOTS, grad_scale,
         ptr(dl), ptr(b[0]), ptr(b[1]), ptr(b[2]), ptr(out), stream())
    return out, dl


def unembed_ce(H, w_pd, b_pd, w_pnd, b_pnd, w_dur, b_dur, plan: Plan, grad_scale=1.0, want_logits=False, out=None,
               dbias=None, dev_scale=None, planes=True):
    """Fused un-embedding + cross-entropy (`pm_unembed_ce`): H [N,15,d] -> (out, d_logits [N,15,230], logits or None)."""
    N, S, d = H.shape
    out = out if out is not None else torch.empty(4, dtype=F64, device=H.device)
    dl = torch.empty(N, S, C.D_TOKEN_PAIR, dtype=F32, device=H.device)
    lg = torch.empty_like(dl) if want_logits else None
    b = dbias if dbias is not None else (None, None, None)
    wpl = torch.empty(int(lib().pm_unembed_scratch_bytes(d)), dtype=torch.uint8, device=H.device) if planes else None
    call("pm_unembed_ce", ptr(H), ptr(w_pd), ptr(b_pd), ptr(w_pnd), ptr(b_pnd), ptr(w_dur), ptr(b_dur), ptr(plan.tokens),
         ptr(plan.buf), N, plan.E, plan.G, d, S, grad_scale, ptr(dev_scale), ptr(lg), ptr(dl), ptr(b[0]), ptr(b[1]), ptr(b[2]),
         ptr(out), ptr(wpl), stream())
    return out, dl, lg


def kld(mu, log_var, out, beta=0.0, dmu=None, dlog_var=None):
    B, d = mu.shape
    call("pm_kld", ptr(mu), ptr(log_var), B, d, beta, ptr(dmu), ptr(dlog_var), ptr(out), stream())
    return out


def bce_logits(logits, target, out, grad_scale=1.0, want_grad=False):
    dl = torch.empty_like(logits) if want_grad else None
    call("pm_bce_logits", ptr(logits), ptr(target), logits.numel(), grad_scale, ptr(dl), ptr(out), stream())
    return out, dl


def content_accuracy(c_logits, tokens, is_drum):
    """Counts of `_accuracies` (training.py:349-468) on the device: int64 [8] =
    {pitch correct, pitch not-PAD, pitch correct (drums), pitch not-PAD (drums), dur correct, dur not-PAD, note correct, 0}."""
    _chk(c_logits, F32, "c_logits"); _chk(tokens, I32, "tokens")
    drum = is_drum.view(U8) if is_drum.dtype == torch.bool else is_drum
    out = torch.empty(8, dtype=I64, device=c_logits.device)
    call("pm_content_accuracy", ptr(c_logits), ptr(tokens), ptr(drum.contiguous()), c_logits.shape[0], ptr(out), stream())
    return out


def content_accuracy_slots(c_logits, tokens, is_drum):
    """`content_accuracy` for logits of the S active slots, [N, S, 230] (`pm_content_accuracy_slots`): int64 [16] in the layout
    of the training-accuracy counts row ([0..7] as `content_accuracy`, the rest 0)."""
    _chk(c_logits, F32, "c_logits"); _chk(tokens, I32, "tokens")
    drum = is_drum.view(U8) if is_drum.dtype == torch.bool else is_drum
    N, S = c_logits.shape[0], c_logits.shape[1]
    verdict = torch.empty(2 * N * S, dtype=U8, device=c_logits.device)
    out = torch.empty(16, dtype=I64, device=c_logits.device)
    call("pm_content_accuracy_slots", ptr(c_logits), ptr(tokens), ptr(drum.contiguous()), N, S, ptr(verdict), ptr(out), stream())
    return out


ACCURACY_KEYS = ("note", "pitch", "pitch_drums", "pitch_non_drums", "dur", "s_acc", "s_precision", "s_recall", "s_f1")


def accuracies_from_counts(c) -> dict:
    """The reference's 9 accuracies (`_accuracies`, training.py:349-497) from one counts row (16 numbers: [0..7] of
    `content_accuracy`, [8..11] of `structure_metrics`, [12] the structure cells).  A zero denominator gives NaN, as the
    reference's 0 / 0; `s_acc` divides by max(cells, 1)."""
    c = [float(v) for v in c]
    m, cells = c[8:12], c[12]
    div = lambda a, b: a / b if b else float("nan")
    prec, rec = div(m[1], m[2]), div(m[1], m[3])
    return {"note": div(c[6], c[1]), "pitch": div(c[0], c[1]), "pitch_drums": div(c[2], c[3]),
            "pitch_non_drums": div(c[0] - c[2], c[1] - c[3]), "dur": div(c[4], c[5]),
            "s_acc": m[0] / max(cells, 1), "s_precision": prec, "s_recall": rec,
            "s_f1": div(2 * rec * prec, rec + prec)}


def structure_metrics(s_logits, s_target):
    """int64 [4] = {prediction == target, true positives, predicted positives, target positives} (training.py:470-497)."""
    _chk(s_logits, F32, "s_logits"); _chk(s_target, F32, "s_target")
    out = torch.empty(4, dtype=I64, device=s_logits.device)
    call("pm_structure_metrics", ptr(s_logits), ptr(s_target), s_logits.numel(), ptr(out), stream())
    return out


def _chk_adam(params, grads, exp_avg, exp_avg_sq):
    for t, n in ((params, "params"), (grads, "grads"), (exp_avg, "exp_avg"), (exp_avg_sq, "exp_avg_sq")):
        _chk(t, F32, n)


def adam_step(params, grads, exp_avg, exp_avg_sq, lr, beta1, beta2, eps, step, grad_scale=1.0):
    _chk_adam(params, grads, exp_avg, exp_avg_sq)
    call("pm_adam_step", ptr(params), ptr(grads), ptr(exp_avg), ptr(exp_avg_sq), params.numel(), lr, beta1, beta2,
         eps, step, grad_scale, stream())


# ---- guarded optimizer step (include/polyphemus_hip.h, "guarded optimizer step"; GradScaler, training.py:160-162)
OVF_WORDS = 8                                   # PM_OVF_WORDS
OVF_PENDING, OVF_LAST, OVF_SNAP, OVF_N_NONFINITE, OVF_N_SATURATED, OVF_STEP_SIZE, OVF_INV_BC2, OVF_TICKET = range(8)
OVF_NONFINITE_BIT, OVF_SATURATED_BIT = 1, 2


def overflow_status(device) -> torch.Tensor:
    """A zeroed status block of the guarded step (int32 [PM_OVF_WORDS], the words read as uint32 by the kernels)."""
    return torch.zeros(OVF_WORDS, dtype=I32, device=device)


def _chk_status(status):
    _chk(status, I32, "status")
    if status.numel() < OVF_WORDS:
        raise ValueError(f"status needs {OVF_WORDS} words")


def _chk_decision(step, skipped):
    if (step is None) != (skipped is None):
        raise ValueError("step and skipped go together")
    if step is not None:
        _chk(step, I64, "step"); _chk(skipped, I64, "skipped")


def overflow_snapshot(status):
    """status[OVF_SNAP] = the pair-format saturation counter, on the current stream (before the step's first split)."""
    _chk_status(status)
    call("pm_overflow_snapshot", ptr(status), stream())


def overflow_poison(grads, status):
    """grads[0] = +inf and the saturation bit in status[OVF_PENDING] if a pair-format split saturated since the snapshot."""
    _chk(grads, F32, "grads"); _chk_status(status)
    call("pm_overflow_poison", ptr(grads), ptr(status), stream())


def grad_nonfinite_check(grads, status, step=None, skipped=None, lr=0.0, beta1=0.0, beta2=0.0, window=False):
    """The non-finite bit in status[OVF_PENDING] if grads holds an inf or a NaN (GradScaler's found_inf).  With the int64
    device words `step` / `skipped` the launch also DECIDES the optimizer step (t + 1 and its Adam scalars, or a skip);
    `window`: a move of the saturation counter since `overflow_snapshot` is a cause too."""
    _chk(grads, F32, "grads"); _chk_status(status); _chk_decision(step, skipped)
    call("pm_grad_nonfinite_check", ptr(grads), grads.numel(), ptr(status), ptr(step), ptr(skipped), lr, beta1, beta2,
         int(bool(window)), stream())


def adam_step_guarded(params, grads, exp_avg, exp_avg_sq, beta1, beta2, eps, status, grad_scale=1.0):
    """`adam_step` at the t and with the scalars `grad_nonfinite_check` decided, unless it decided a skip: then nothing is
    stored.  An applied step equals `adam_step` at that t bit for bit."""
    _chk_adam(params, grads, exp_avg, exp_avg_sq)
    _chk_status(status)
    call("pm_adam_step_guarded", ptr(params), ptr(grads), ptr(exp_avg), ptr(exp_avg_sq), params.numel(), beta1, beta2,
         eps, grad_scale, ptr(status), stream())


def adam_bias_scalars(steps, lr, beta1, beta2):
    """[n, 2] float32: (lr / (1 - beta1^t), 1 / sqrt(1 - beta2^t)) for each t of the int64 device tensor `steps`, from the
    device function the step's decision uses."""
    _chk(steps, I64, "steps")
    out = torch.empty(steps.numel(), 2, dtype=F32, device=steps.device)
    call("pm_adam_bias_scalars", ptr(steps), steps.numel(), lr, beta1, beta2, ptr(out), stream())
    return out


# ---- gradient clipping by the global norm (include/polyphemus_hip.h, "gradient clipping by the global norm")
CLIP_NORM, CLIP_COEF, CLIP_GSCALE, CLIP_SUMSQ, CLIP_PARTIALS_AT = range(5)   # PM_CLIP_*
CLIP_PARTIALS = 256                             # PM_CLIP_PARTIALS
CLIP_WORDS = 260                                # PM_CLIP_WORDS


def clip_block(device) -> torch.Tensor:
    """A clip block (float64 [PM_CLIP_WORDS]: norm, coef, gscale, sumsq, then the per-workgroup partials)."""
    return torch.zeros(CLIP_WORDS, dtype=F64, device=device)


def _chk_clip(clip):
    _chk(clip, F64, "clip")
    if clip.numel() < CLIP_WORDS:
        raise ValueError(f"clip needs {CLIP_WORDS} doubles")


def grad_sumsq(grads, clip):
    """The per-workgroup sums of squares of `grads` (squared and added in double, a fixed order) into the partials of `clip`."""
    _chk(grads, F32, "grads"); _chk_clip(clip)
    call("pm_grad_sumsq", ptr(grads), grads.numel(), ptr(clip), stream())


def grad_nonfinite_check_sumsq(grads, status, clip, step=None, skipped=None, lr=0.0, beta1=0.0, beta2=0.0, window=False):
    """`grad_nonfinite_check` and `grad_sumsq` in one read of the gradient."""
    _chk(grads, F32, "grads"); _chk_status(status); _chk_clip(clip); _chk_decision(step, skipped)
    call("pm_grad_nonfinite_check_sumsq", ptr(grads), grads.numel(), ptr(status), ptr(step), ptr(skipped), lr, beta1, beta2,
         int(bool(window)), ptr(clip), stream())


def grad_clip_finish(clip, max_norm, grad_scale=1.0, row=None):
    """From the partials: norm = |grad_scale| * sqrt(sum), coef = min(1, max_norm / (norm + 1e-6)) — the formula of
    `torch.nn.utils.clip_grad_norm_` — and gscale = float32(grad_scale * coef) into `clip`; (norm, coef) into the float64
    pair `row` if given.  `max_norm` = inf measures only."""
    _chk_clip(clip)
    if row is not None:
        _chk(row, F64, "row")
        if row.numel() < 2:
            raise ValueError("row needs 2 doubles")
    call("pm_grad_clip_finish", ptr(clip), grad_scale, max_norm, ptr(row), stream())


def adam_step_clipped(params, grads, exp_avg, exp_avg_sq, lr, beta1, beta2, eps, step, clip, status=None):
    """`adam_step` (or, with the guarded step's `status`, `adam_step_guarded`: `lr` and `step` are then unused) with the
    gradient scale `grad_clip_finish` left in `clip`.  Unclipped (coef == 1) it equals them bit for bit."""
    _chk_adam(params, grads, exp_avg, exp_avg_sq)
    _chk_clip(clip)
    if status is not None:
        _chk_status(status)
    call("pm_adam_step_clipped", ptr(params), ptr(grads), ptr(exp_avg), ptr(exp_avg_sq), params.numel(), lr, beta1, beta2,
         eps, step, ptr(clip), ptr(status), stream())


# ---- exponential moving average of the parameters (include/polyphemus_hip.h, "exponential moving average of the parameters")
def ema_weight(decay) -> float:
    """The weight of the fresh parameter in the average as the kernel takes it: float32(1 - decay), the difference formed in
    double.  ValueError unless `decay` is a number (not a bool) in [0, 1) that is still below 1 as a float32: past that the
    weight is under 2^-25, where ema + weight * (p - ema) rounds back to ema for every p within a factor of two of it (and
    under 1.4e-45 the weight itself rounds to 0) — an average that never moves."""
    if isinstance(decay, bool) or not isinstance(decay, (int, float)) or not 0.0 <= decay < 1.0:
        raise ValueError(f"ema_decay must be None or a number in [0, 1), not {decay!r}")
    w = ctypes.c_float(1.0 - float(decay)).value
    if not ctypes.c_float(decay).value < 1.0 or not 0.0 < w <= 1.0:
        raise ValueError(f"ema_decay = {decay!r} is 1 as a float32 (weight {w!r}): the average would never move")
    return w


def adam_step_ema(params, grads, exp_avg, exp_avg_sq, ema, lr, beta1, beta2, eps, step, ema_weight, grad_scale=1.0, clip=None,
                  status=None):
    """`adam_step` (or, with `clip` / `status`, `adam_step_clipped` / `adam_step_guarded`: the same bits in params and both
    moments) that also moves `ema` towards the parameter it stored: ema += ema_weight * (params - ema), a copy at
    ema_weight == 1.  A skipped step leaves `ema` alone."""
    _chk_adam(params, grads, exp_avg, exp_avg_sq)
    _chk(ema, F32, "ema")
    if ema.numel() != params.numel():
        raise ValueError("ema must have as many elements as params")
    if not 0.0 < ema_weight <= 1.0:
        raise ValueError(f"ema_weight must be in (0, 1], not {ema_weight!r}")
    if clip is not None:
        _chk_clip(clip)
    if status is not None:
        _chk_status(status)
    call("pm_adam_step_ema", ptr(params), ptr(grads), ptr(exp_avg), ptr(exp_avg_sq), ptr(ema), params.numel(), lr, beta1,
         beta2, eps, step, grad_scale, ema_weight, ptr(clip), ptr(status), stream())


def buffer_swap(a, b):
    """a <-> b in place (two fp32 buffers of one size that do not overlap)."""
    _chk(a, F32, "a"); _chk(b, F32, "b")
    if a.numel() != b.numel():
        raise ValueError("a and b must have the same number of elements")
    call("pm_buffer_swap", ptr(a), ptr(b), a.numel(), stream())
