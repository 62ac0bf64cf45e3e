"""Dataset + device-side collate: the input side of the hot path.

The reference's `PolyphemusDataset.__getitem__` (data.py:218-271) expands every sample to one-hot `c_tensor`s
(14.7 KB per node) and builds its bar graphs with Python loops on the host (6-170 ms per sample), then PyG's collate
concatenates them (train.py:152).  Here a sample stays in its on-disk form — token ids int16 [nb,4,32,16,2] and the
activation grid [nb,4,32] (preprocess.py:118-149,210) — a batch is two pinned host arrays (4.2 MB + 64 KB at B = 256),
one H2D copy each on a side stream, and the batch of bar graphs is built ON THE DEVICE (`csrc/graph.hip`) with the
reference's node numbering and edge order, so the result is interchangeable bit for bit with the reference's
DataLoader output (tests/test_data_gpu.py on the samples the reference itself collated).
"""
from __future__ import annotations

import os
from concurrent.futures import ThreadPoolExecutor
from typing import Iterator, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import constants as C
from .graphs import BarGraphBatch, device_batch_from_structure


class PolyphemusDataset:
    """Mirror of the reference's `PolyphemusDataset(dir, n_bars)` (data.py:206-216) over the same `.npz` files
    (`c_tensor` int [4, nb*32, 16, 2], `s_tensor` bool [4, nb*32]).  `__getitem__` returns the sample re-laid out bar
    by bar (data.py:226-233) as token ids; no one-hots, no graph — those are the device's job.  Files are taken in
    sorted order (the reference uses `os.scandir` order, which is arbitrary)."""

    def __init__(self, dir: str, n_bars: int = 2):
        self.dir = dir
        self.files = sorted(e.name for e in os.scandir(dir) if e.is_file())
        self.len = len(self.files)
        self.n_bars = n_bars

    def __len__(self) -> int:
        return self.len

    def __getitem__(self, idx: int) -> Tuple[np.ndarray, np.ndarray]:
        with np.load(os.path.join(self.dir, self.files[idx])) as data:
            return relayout_sample(data["c_tensor"], data["s_tensor"], self.n_bars)


def relayout_sample(c_disk: np.ndarray, s_disk: np.ndarray, n_bars: int) -> Tuple[np.ndarray, np.ndarray]:
    """(n_tracks x n_bars*32 x ...) -> (n_bars x n_tracks x 32 x ...), data.py:226-233: token grid int16
    [nb,4,32,16,2] and activation grid uint8 [nb,4,32]."""
    if c_disk.shape != (C.N_TRACKS, n_bars * C.N_TIMESTEPS, C.MAX_SIMU_TOKENS, 2):
        raise ValueError(f"c_tensor has shape {c_disk.shape}, expected {(C.N_TRACKS, n_bars * C.N_TIMESTEPS, C.MAX_SIMU_TOKENS, 2)}")
    if s_disk.shape != (C.N_TRACKS, n_bars * C.N_TIMESTEPS):
        raise ValueError(f"s_tensor has shape {s_disk.shape}, expected {(C.N_TRACKS, n_bars * C.N_TIMESTEPS)}")
    c = c_disk.reshape(C.N_TRACKS, n_bars, C.N_TIMESTEPS, C.MAX_SIMU_TOKENS, 2).transpose(1, 0, 2, 3, 4)
    s = s_disk.reshape(C.N_TRACKS, n_bars, C.N_TIMESTEPS).transpose(1, 0, 2)
    return np.ascontiguousarray(c, dtype=np.int16), np.ascontiguousarray(s, dtype=np.uint8)


def collate_on_device(samples: Sequence[Tuple[np.ndarray, np.ndarray]], n_bars: int, device="cuda",
                      staging: Optional[Tuple[torch.Tensor, torch.Tensor]] = None) -> BarGraphBatch:
    """Batch of `PolyphemusDataset` samples -> the `BarGraphBatch` the reference's DataLoader would deliver
    (PyG collate of the per-sample graphs), built on the device.  `staging` = optional pinned host
    buffers (token grid int16 [>=B,nb,4,32,16,2], structure uint8 [>=B,nb,4,32]) to copy through."""
    B = len(samples)
    if B == 0:
        raise ValueError("empty batch")
    if staging is None:
        staging = _staging(B, n_bars, pin=False)
    tok_h, s_h = staging[0][:B], staging[1][:B]
    for i, (c, s) in enumerate(samples):
        tok_h[i] = torch.from_numpy(c)
        s_h[i] = torch.from_numpy(s)
    # active token slots of the batch (`PmBatch.n_slots`): the last slot that holds a non-PAD token in any ACTIVE cell
    # (an empty bar's cell [0,0] counts: the graph builder switches it on, data.py:152-153) — 4 MB of int16 on the host
    s_np, tok_np = s_h.numpy().astype(bool), tok_h.numpy()
    empty = ~s_np.any(axis=(-1, -2))
    if empty.any():
        s_np = s_np.copy()
        s_np[..., 0, 0] |= empty
    live = ((tok_np[..., 1:, 0] != C.PITCH_PAD) | (tok_np[..., 1:, 1] != C.DUR_PAD)) & s_np[..., None]
    slots = np.nonzero(live.reshape(-1, C.MAX_SIMU_TOKENS - 1).any(axis=0))[0]
    tok = tok_h.to(device, non_blocking=True)
    s = s_h.to(device, non_blocking=True)
    batch = device_batch_from_structure(s.view(B * n_bars, C.N_TRACKS, C.N_TIMESTEPS), n_bars, token_grid=tok)
    batch.n_slots = int(slots.max()) + 1 if slots.size else 1
    return batch


def _staging(B: int, n_bars: int, pin: bool):
    tok = torch.empty(B, n_bars, C.N_TRACKS, C.N_TIMESTEPS, C.MAX_SIMU_TOKENS, 2, dtype=torch.int16)
    s = torch.empty(B, n_bars, C.N_TRACKS, C.N_TIMESTEPS, dtype=torch.uint8)
    return (tok.pin_memory(), s.pin_memory()) if pin else (tok, s)


def _rank_and_world(rank: Optional[int], world: Optional[int]) -> Tuple[int, int]:
    """(rank, world) of a loader: the arguments, else the torch.distributed default group, else (0, 1)"""
    import torch.distributed as dist
    ddp = dist.is_available() and dist.is_initialized()
    rank = int(rank) if rank is not None else (dist.get_rank() if ddp else 0)
    world = int(world) if world is not None else (dist.get_world_size() if ddp else 1)
    if not 0 <= rank < world:
        raise ValueError(f"rank {rank} outside world {world}")
    return rank, world


def shard_len(n: int, world: int) -> int:
    """samples per rank and epoch: every rank gets the same number (wrap-around padding)"""
    return (n + world - 1) // world


def n_batches(n: int, batch_size: int, drop_last: bool, world: int) -> int:
    m = shard_len(n, world)
    return m // batch_size if drop_last else (m + batch_size - 1) // batch_size


def index_batches(n: int, batch_size: int, shuffle: bool, seed: int, epoch: int, drop_last: bool, rank: int,
                  world: int) -> List[np.ndarray]:
    """The sample indices of one rank's batches in one epoch, shared by `DeviceLoader` and `ResidentLoader` so that the
    two cannot drift: the permutation of `default_rng(seed + epoch)` (every rank draws the SAME one), padded by
    wrap-around to a multiple of `world`, every world-th index starting at `rank`, cut into batches."""
    order = np.random.default_rng(seed + epoch).permutation(n) if shuffle else np.arange(n)
    if world > 1:
        total = shard_len(n, world) * world
        # DistributedSampler's rule: wrap around — repeatedly when the dataset is smaller than the world (np.resize
        # tiles) — so that every rank gets the same number of samples and batches: the all-reduce needs lock step
        order = np.resize(order, total)[rank::world]
        n = order.shape[0]
    out = [order[i:i + batch_size] for i in range(0, n, batch_size)]
    if drop_last and out and len(out[-1]) < batch_size:
        out.pop()
    return out


class DeviceLoader:
    """`DataLoader(dataset, batch_size, shuffle)` of train.py:152-156 with the collate on the device.  Batches are
    staged through two sets of pinned host buffers and copied + built on a side stream one batch ahead of the
    consumer: file reading (`num_workers` threads), the H2D copy and the graph kernels of batch i+1 overlap the
    (asynchronous) training step of batch i.  Partial last batches are kept (`drop_last=False`, the DataLoader default
    the reference uses)."""

    def __init__(self, dataset, batch_size: int, shuffle: bool = False, seed: int = 0, device="cuda",
                 drop_last: bool = False, num_workers: int = 0, rank: Optional[int] = None, world: Optional[int] = None):
        """`batch_size` is PER RANK.  Under data parallelism (`rank` / `world`, default: the torch.distributed default
        group) the loader behaves like `DistributedSampler`: every rank draws the SAME permutation (seed + epoch),
        pads it by wrap-around to a multiple of `world` and keeps every world-th index starting at its rank — disjoint
        shards, the same number of batches on every rank (the gradient all-reduce needs the ranks in lock step)."""
        self.rank, self.world = _rank_and_world(rank, world)
        self.dataset, self.batch_size, self.shuffle, self.seed = dataset, int(batch_size), shuffle, seed
        self.device, self.drop_last = torch.device(device), drop_last
        self._pool = ThreadPoolExecutor(num_workers) if num_workers > 0 else None
        self.n_bars = dataset.n_bars
        self.epoch = 0
        self._stage = [_staging(self.batch_size, self.n_bars, pin=True) for _ in range(2)]
        self._stream = torch.cuda.Stream(device=self.device)

    def _shard_len(self) -> int:
        return shard_len(len(self.dataset), self.world)

    def __len__(self) -> int:
        return n_batches(len(self.dataset), self.batch_size, self.drop_last, self.world)

    def _index_batches(self) -> List[np.ndarray]:
        return index_batches(len(self.dataset), self.batch_size, self.shuffle, self.seed, self.epoch, self.drop_last,
                             self.rank, self.world)

    def _build(self, idx: np.ndarray, slot: int):
        """enqueue copy + graph construction of one batch on the side stream; returns (batch, ready event)"""
        if self._pool is not None:
            samples = list(self._pool.map(self.dataset.__getitem__, [int(i) for i in idx]))
        else:
            samples = [self.dataset[int(i)] for i in idx]
        with torch.cuda.stream(self._stream):
            batch = collate_on_device(samples, self.n_bars, self.device, self._stage[slot])
            ev = torch.cuda.Event()
            ev.record(self._stream)
        return batch, ev

    def __iter__(self) -> Iterator[BarGraphBatch]:
        batches = self._index_batches()
        self.epoch += 1
        if not batches:
            return
        nxt = self._build(batches[0], 0)
        for j in range(len(batches)):
            batch, ev = nxt
            # `device_batch_from_structure` reads (N, E) back, so the side stream has finished this batch's copy: the
            # other staging slot is free to be refilled while the consumer trains on `batch`
            if j + 1 < len(batches):
                nxt = self._build(batches[j + 1], (j + 1) & 1)
            torch.cuda.current_stream(self.device).wait_event(ev)
            for v in batch.__dict__.values():
                if torch.is_tensor(v) and v.is_cuda:
                    v.record_stream(torch.cuda.current_stream(self.device))
            yield batch


def _bit_planes(s_bits: torch.Tensor) -> torch.Tensor:
    """masks int32 [...] -> 0/1 uint8 [..., 32] (bit t of a word at position t); plain torch, off the hot path"""
    steps = torch.arange(C.N_TIMESTEPS, dtype=torch.int32, device=s_bits.device)
    return ((s_bits.unsqueeze(-1) >> steps) & 1).to(torch.uint8)


class ResidentDataset:
    """A whole data set on the device in compact form ("Resident data set" in include/polyphemus_hip.h, csrc/dataset.hip),
    from which a batch is a gather by index: no file, no dense grid, no host pass and no host read per batch.

      s_bits   int32 [n, n_bars, 4]   bit t of word (bar, track): the cell is active (the empty-bar rule applied)
      rows     uint8 [R, 16, 2]       token rows (pitch id, duration id) of the active cells in node order
      cell_ptr int64 [n + 1]          row offsets per sample
    and on the host, 12 B per sample: nodes, edges and the last live token slot, from which N, E and `n_slots` of any index
    list are host arithmetic.  32 B per active cell plus 16 B per bar: about 2 KB per two-bar sample."""

    def __init__(self, s_bits: torch.Tensor, rows: torch.Tensor, cell_ptr: torch.Tensor, nodes, edges, last_slot, n_bars: int):
        from . import ops
        n, R = ops._dataset_store_args(s_bits, rows, cell_ptr, n_bars)
        counts = []
        for a, name in ((nodes, "nodes"), (edges, "edges"), (last_slot, "last_slot")):
            a = np.asarray(a)
            if a.shape != (n,) or a.dtype.kind not in "iu":
                raise ValueError(f"{name} must be an integer array [n = {n}], got {a.dtype} {a.shape}")
            counts.append(np.ascontiguousarray(a, dtype=np.int32))
        self._nodes, self._edges, self._last = counts
        if self._nodes.min() < n_bars or self._nodes.max() > 128 * n_bars or int(self._nodes.sum(dtype=np.int64)) != R:
            raise ValueError(f"nodes: every sample holds {n_bars}..{128 * n_bars} cells and all of them the {R} rows")
        if self._edges.min() < n_bars:
            raise ValueError(f"edges: every sample holds at least {n_bars} edges")
        if self._last.min() < 0 or self._last.max() > C.MAX_SIMU_TOKENS - 1:
            raise ValueError(f"last_slot: entries lie in [0, {C.MAX_SIMU_TOKENS - 1}]")
        for t, name in ((rows, "rows"), (cell_ptr, "cell_ptr")):
            if t.device != s_bits.device:
                raise ValueError(f"{name} lives on {t.device}, s_bits on {s_bits.device}")
        self.s_bits, self.rows, self.cell_ptr = s_bits.contiguous(), rows.contiguous(), cell_ptr.contiguous()
        self.n_bars = int(n_bars)

    # -- construction ----------------------------------------------------------------------------------------------
    @classmethod
    def _from_chunks(cls, chunks, n_bars: int) -> "ResidentDataset":
        """`chunks` yields (token_grid int16 [c,nb,4,32,16,2], s_grid uint8 [c,nb,4,32]) on the device; each is packed
        behind the rows of those before it, so the store does not depend on where the chunks were cut"""
        from . import ops
        bits, nodes, edges, last = [], [], [], []
        rows, R = None, 0
        for tok, s in chunks:
            out = ops.dataset_pack(tok, s, rows, R)
            rows, R = out["rows"], R + out["total"]
            bits.append(out["s_bits"]); nodes.append(out["cells"]); edges.append(out["edges"]); last.append(out["last_slot"])
        if not bits:
            raise ValueError("empty data set")
        nodes = np.concatenate(nodes)
        cell_ptr = np.zeros(nodes.shape[0] + 1, np.int64)
        np.cumsum(nodes, out=cell_ptr[1:])
        rows = rows if rows.shape[0] == R else rows[:R].clone()          # (lets the over-allocation go)
        return cls(torch.cat(bits), rows, torch.from_numpy(cell_ptr).to(rows.device), nodes, np.concatenate(edges),
                   np.concatenate(last), n_bars)

    @staticmethod
    def _check_chunk(chunk) -> int:
        if isinstance(chunk, (bool, np.bool_)) or not isinstance(chunk, (int, np.integer)) or chunk < 1:
            raise ValueError(f"chunk must be an int >= 1, got {chunk!r}")
        return int(chunk)

    @classmethod
    def from_arrays(cls, token_grid, s_grid, device="cuda", chunk: int = 1024) -> "ResidentDataset":
        """From the samples as `PolyphemusDataset` delivers them, stacked: `token_grid` int16 [n,nb,4,32,16,2] and `s_grid`
        uint8 [n,nb,4,32] (numpy arrays or tensors), packed on `device` `chunk` samples at a time."""
        tok, s = torch.as_tensor(token_grid), torch.as_tensor(s_grid)
        if s.dtype == torch.bool:
            s = s.to(torch.uint8)
        if tok.dtype != torch.int16 or tok.dim() != 6 or tok.shape[0] < 1 or tok.shape[1] < 1 or \
                tuple(tok.shape[2:]) != (C.N_TRACKS, C.N_TIMESTEPS, C.MAX_SIMU_TOKENS, 2):
            raise ValueError(f"token_grid must be int16 [n,n_bars,4,32,16,2], got {tok.dtype} {tuple(tok.shape)}")
        if s.dtype != torch.uint8 or tuple(s.shape) != tuple(tok.shape[:4]):
            raise ValueError(f"s_grid must be uint8 {tuple(tok.shape[:4])}, got {s.dtype} {tuple(s.shape)}")
        chunk = cls._check_chunk(chunk)
        return cls._from_chunks(((tok[a:a + chunk].to(device), s[a:a + chunk].to(device)) for a in range(0, tok.shape[0], chunk)),
                                int(tok.shape[1]))

    @classmethod
    def from_dataset(cls, dataset, device="cuda", chunk: int = 1024, num_workers: int = 0) -> "ResidentDataset":
        """From a `PolyphemusDataset` (anything with `n_bars`, `len` and `[i] -> (token grid, structure)`): the samples are
        read `chunk` at a time (`num_workers` threads) through one pinned staging pair and packed on the device."""
        chunk, n = cls._check_chunk(chunk), len(dataset)
        if n < 1:
            raise ValueError("empty data set")
        chunk = min(chunk, n)
        pin = torch.device(device).type == "cuda"
        tok_h, s_h = _staging(chunk, dataset.n_bars, pin=pin)
        pool = ThreadPoolExecutor(num_workers) if num_workers > 0 else None

        def chunks():
            for a in range(0, n, chunk):
                ids = range(a, min(a + chunk, n))
                samples = pool.map(dataset.__getitem__, ids) if pool is not None else (dataset[i] for i in ids)
                for k, (c, s) in enumerate(samples):
                    tok_h[k] = torch.from_numpy(c)
                    s_h[k] = torch.from_numpy(s)
                # (packing ends with a host read, so the staging pair is free again when the next chunk is filled)
                yield tok_h[:len(ids)].to(device, non_blocking=True), s_h[:len(ids)].to(device, non_blocking=True)
        try:
            return cls._from_chunks(chunks(), dataset.n_bars)
        finally:
            if pool is not None:
                pool.shutdown()

    @classmethod
    def from_notes(cls, note_batch, chunk: int = 1024) -> "ResidentDataset":
        """The pieces of a `NoteBatch` as the samples, for instance the windows of `NoteBatch.windows(n_bars,
        filter="reference")`, on the batch's device: `ops.tokens_from_notes` per chunk of pieces, its node rows laid back
        into a token grid with torch (this runs once), then packed like any other chunk."""
        from . import ops
        notes, track_ptr, nb = note_batch.notes, note_batch.track_ptr, int(note_batch.n_bars)
        chunk, dev = cls._check_chunk(chunk), notes.device
        ptr_h = track_ptr.cpu()
        B = (ptr_h.shape[0] - 1) // 4

        def chunks():
            for a in range(0, B, chunk):
                b = min(a + chunk, B)
                lo, hi = int(ptr_h[4 * a]), int(ptr_h[4 * b])
                s, tokens, _ = ops.tokens_from_notes(notes[lo:hi], (ptr_h[4 * a:4 * b + 1] - lo).to(dev), nb)
                grid = torch.zeros((b - a) * nb * 128, C.MAX_SIMU_TOKENS, 2, dtype=torch.int16, device=dev)
                grid[s.reshape(-1) != 0] = tokens.to(torch.int16)
                yield (grid.view(b - a, nb, C.N_TRACKS, C.N_TIMESTEPS, C.MAX_SIMU_TOKENS, 2),
                       s.view(b - a, nb, C.N_TRACKS, C.N_TIMESTEPS).to(torch.uint8))
        return cls._from_chunks(chunks(), nb)

    # -- I/O -------------------------------------------------------------------------------------------------------
    def save(self, path: str) -> None:
        """One `.npz` with the compact arrays and the per-sample counts"""
        with open(path, "wb") as f:
            np.savez(f, s_bits=self.s_bits.cpu().numpy().view(np.uint32), rows=self.rows.cpu().numpy(),
                     cell_ptr=self.cell_ptr.cpu().numpy(), nodes=self._nodes, edges=self._edges, last_slot=self._last,
                     n_bars=np.int32(self.n_bars))

    @classmethod
    def load(cls, path: str, device="cuda") -> "ResidentDataset":
        """The store `save` wrote.  The counts decide output sizes nobody reads back later, so they are checked against
        the arrays once here: the masks' popcounts, `cell_ptr`, and on the device the edges (`pm_graph_count`)."""
        with np.load(path) as z:
            missing = [k for k in ("s_bits", "rows", "cell_ptr", "nodes", "edges", "last_slot", "n_bars") if k not in z.files]
            if missing:
                raise ValueError(f"{path}: not a resident data set (no {', '.join(missing)})")
            a = {k: z[k] for k in z.files}
        if a["s_bits"].dtype != np.uint32:
            raise ValueError(f"{path}: s_bits must be uint32, got {a['s_bits'].dtype}")
        self = cls(torch.from_numpy(a["s_bits"].view(np.int32)).to(device), torch.from_numpy(a["rows"]).to(device),
                   torch.from_numpy(a["cell_ptr"]).to(device), a["nodes"], a["edges"], a["last_slot"], int(a["n_bars"]))
        words = a["s_bits"].reshape(len(self), -1)
        cells = sum(((words >> np.uint32(t)) & np.uint32(1)).sum(axis=1, dtype=np.int64) for t in range(32))
        ptr = np.zeros(len(self) + 1, np.int64)
        np.cumsum(self._nodes, out=ptr[1:])
        if not (np.array_equal(cells, self._nodes) and np.array_equal(ptr, a["cell_ptr"])):
            raise ValueError(f"{path}: nodes, cell_ptr and the masks of s_bits do not agree")
        if not np.array_equal(self._count_edges(), self._edges):
            raise ValueError(f"{path}: edges do not agree with the masks of s_bits")
        return self

    def _count_edges(self, chunk: int = 4096) -> np.ndarray:
        """edges per sample from the masks, on the device (`pm_graph_count`), int32 [n]"""
        from ._lib import HipExtensionError, call, ptr, stream
        if not self.s_bits.is_cuda:
            raise HipExtensionError(f"the store lives on {self.s_bits.device}: the HIP path needs device tensors (no CPU fallback)")
        out, nb, dev = [], self.n_bars, self.s_bits.device
        for a in range(0, len(self), chunk):
            s = _bit_planes(self.s_bits[a:a + chunk]).to(torch.float32).view(-1, C.N_TRACKS, C.N_TIMESTEPS).contiguous()
            G = s.shape[0]
            bn, be = torch.empty(G, dtype=torch.int32, device=dev), torch.empty(G, dtype=torch.int32, device=dev)
            scan = torch.empty(2 * G + 4, dtype=torch.int32, device=dev)
            call("pm_graph_count", ptr(s), G, ptr(bn), ptr(be), ptr(scan), ptr(scan[G + 1:]), ptr(scan[2 * G + 2:]), stream())
            out.append(be.view(-1, nb).sum(dim=1, dtype=torch.int32).cpu().numpy())
        return np.concatenate(out)

    # -- the store ---------------------------------------------------------------------------------------------------
    def __len__(self) -> int:
        return int(self.s_bits.shape[0])

    @property
    def device(self) -> torch.device:
        return self.s_bits.device

    @property
    def nbytes(self) -> int:
        """bytes of the store on the device"""
        return sum(int(t.numel()) * t.element_size() for t in (self.s_bits, self.rows, self.cell_ptr))

    def __eq__(self, other) -> bool:
        return isinstance(other, ResidentDataset) and self.n_bars == other.n_bars and \
            all(a.shape == b.shape and bool((a.cpu() == b.cpu()).all())
                for a, b in ((self.s_bits, other.s_bits), (self.rows, other.rows), (self.cell_ptr, other.cell_ptr))) and \
            all(np.array_equal(a, b) for a, b in ((self._nodes, other._nodes), (self._edges, other._edges), (self._last, other._last)))

    __hash__ = None

    # -- batches -----------------------------------------------------------------------------------------------------
    def _check_index(self, index) -> np.ndarray:
        if isinstance(index, torch.Tensor):
            if index.is_cuda:
                raise ValueError("index must live on the host (a list, a numpy array or a CPU tensor of ints)")
            index = index.numpy()
        elif isinstance(index, range):
            index = np.arange(index.start, index.stop, index.step)
        elif isinstance(index, (list, tuple)):
            if not all(isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_)) for v in index):
                raise ValueError(f"index must hold ints, got {index!r}")
            index = np.asarray(index, dtype=np.int64) if len(index) else np.zeros(0, np.int64)
        if not isinstance(index, np.ndarray) or index.dtype.kind not in "iu" or index.ndim != 1 or index.shape[0] < 1:
            raise ValueError("index must be a non-empty list, numpy array [B] or CPU tensor [B] of ints")
        index = index.astype(np.int64)
        bad = (index < 0) | (index >= len(self))
        if bad.any():
            raise ValueError(f"index: {int(bad.sum())} entries outside [0, {len(self)})")
        return index

    @staticmethod
    def _check_transpose(transpose, B: int) -> Optional[np.ndarray]:
        if transpose is None:
            return None
        if isinstance(transpose, torch.Tensor):
            if transpose.is_cuda:
                raise ValueError("transpose must live on the host (a list, a numpy array or a CPU tensor of ints)")
            transpose = transpose.numpy()
        t = np.asarray(transpose)
        if t.dtype.kind not in "iu" or t.shape != (B,):
            raise ValueError(f"transpose must be None or ints [B = {B}], got {t.dtype} {t.shape}")
        if (np.abs(t.astype(np.int64)) > 127).any():
            raise ValueError("transpose: a shift beyond +-127 semitones")
        return t.astype(np.int32)

    def batch(self, index, transpose=None, check: bool = False) -> BarGraphBatch:
        """The `BarGraphBatch` of the samples `index` (host ints, repeats allowed) in that order: what `collate_on_device`
        builds from the same samples, key for key, plus `transpose` (the shifts on the device, or None).  `transpose` holds
        one shift in semitones per entry (host ints, |shift| <= 127): the reference's rule (preprocess.py:196-205: tracks
        1..3, not SOS / EOS / PAD, clipped to 0..127) applied while gathering.  N, E, the row offsets and `n_slots` come
        from the host copies of the counts; they and the index reach the device in one small non-blocking copy, the batch
        is one gather launch and `graph_build` with the sizes given: NO host read.  `check` reads the gather's status and
        `graph_build`'s device totals back (one host read) and raises ValueError when either disagrees with the host."""
        from . import ops
        from ._lib import HipExtensionError
        idx = self._check_index(index)
        B = idx.shape[0]
        shifts = self._check_transpose(transpose, B)
        out_ptr = np.zeros(B + 1, np.int64)
        np.cumsum(self._nodes[idx], out=out_ptr[1:])
        N, E = int(out_ptr[-1]), int(self._edges[idx].sum(dtype=np.int64))
        if N > 0x7fffffff or E > 0x7fffffff:
            raise ValueError(f"index: the batch holds {N} nodes and {E} edges, beyond 2^31")
        if not self.s_bits.is_cuda:
            raise HipExtensionError(f"the store lives on {self.s_bits.device}: the HIP path needs device tensors (no CPU fallback)")
        host = torch.empty(3 * B + 1, dtype=torch.int32, pin_memory=True)
        h = host.numpy()
        h[:B], h[B:2 * B + 1] = idx, out_ptr
        h[2 * B + 1:] = 0 if shifts is None else shifts
        dev = host.to(self.s_bits.device, non_blocking=True)
        shift_d = None if shifts is None else dev[2 * B + 1:]
        s, tokens, status = ops.dataset_gather(self.s_bits, self.rows, self.cell_ptr, self.n_bars, dev[:B], dev[B:2 * B + 1], N,
                                               shift_d)
        g = ops.graph_build(s, self.n_bars, sizes=(N, E))
        if check:
            out_of_range, mismatched, n_dev, e_dev = torch.cat([status, g["totals"]]).tolist()      # the one host read
            if out_of_range or mismatched or (n_dev, e_dev) != (N, E):
                raise ValueError(f"index: {out_of_range} entries outside the store, {mismatched} whose rows do not match the "
                                 f"store; the device counts ({n_dev}, {e_dev}) nodes and edges, the host ({N}, {E})")
        return BarGraphBatch(n_slots=max(1, int(self._last[idx].max())), track_unique=True, edge_index=g["edge_index"],
                             edge_type=g["edge_type"], edge_dist=g["edge_dist"], s_tensor=s, is_drum=g["is_drum"],
                             bars=g["bars"], batch=g["batch"], num_nodes=N, n_bars=self.n_bars, node_cell=g["node_cell"],
                             tokens=tokens, transpose=shift_d)


class ResidentLoader:
    """`DeviceLoader` over a `ResidentDataset`: the same epochs, permutations, shards and batches (`index_batches`), with
    nothing on the host per batch but index arithmetic.  Batches are enqueued `prefetch` ahead on a side stream — nothing is
    read back, so that is only enqueueing — and handed over with an event wait and `record_stream`.  `transpose="random"`
    draws one shift in -5..6 semitones per sample and epoch (`default_rng([seed, epoch, rank])`), the augmentation the
    reference bakes into its files once; None gives the stored pitches."""

    def __init__(self, resident: ResidentDataset, batch_size: int, shuffle: bool = False, seed: int = 0, drop_last: bool = False,
                 rank: Optional[int] = None, world: Optional[int] = None, transpose=None, prefetch: int = 2):
        if not isinstance(resident, ResidentDataset):
            raise ValueError(f"resident must be a ResidentDataset, got {type(resident).__name__}")
        if isinstance(batch_size, (bool, np.bool_)) or not isinstance(batch_size, (int, np.integer)) or batch_size < 1:
            raise ValueError(f"batch_size must be an int >= 1, got {batch_size!r}")
        if transpose not in (None, "random"):
            raise ValueError(f"transpose must be None or 'random', got {transpose!r}")
        if isinstance(prefetch, (bool, np.bool_)) or not isinstance(prefetch, (int, np.integer)) or prefetch < 1:
            raise ValueError(f"prefetch must be an int >= 1, got {prefetch!r}")
        self.rank, self.world = _rank_and_world(rank, world)
        self.resident, self.batch_size, self.shuffle, self.seed = resident, int(batch_size), shuffle, seed
        self.drop_last, self.transpose, self.prefetch = drop_last, transpose, int(prefetch)
        self.n_bars, self.device = resident.n_bars, resident.device
        self.epoch = 0
        self._stream = torch.cuda.Stream(device=self.device) if self.device.type == "cuda" else None

    def __len__(self) -> int:
        return n_batches(len(self.resident), self.batch_size, self.drop_last, self.world)

    def _index_batches(self) -> List[np.ndarray]:
        return index_batches(len(self.resident), self.batch_size, self.shuffle, self.seed, self.epoch, self.drop_last,
                             self.rank, self.world)

    def _shifts(self, batches: List[np.ndarray]) -> List[Optional[np.ndarray]]:
        if self.transpose is None:
            return [None] * len(batches)
        drawn = np.random.default_rng([self.seed, self.epoch, self.rank]).integers(-5, 7, size=sum(len(b) for b in batches))
        ends = np.cumsum([len(b) for b in batches])
        return [drawn[e - len(b):e].astype(np.int32) for b, e in zip(batches, ends)]

    def __iter__(self) -> Iterator[BarGraphBatch]:
        from collections import deque
        from ._lib import HipExtensionError
        if self._stream is None:
            raise HipExtensionError(f"the store lives on {self.device}: the HIP path needs device tensors (no CPU fallback)")
        batches = self._index_batches()
        shifts = self._shifts(batches)
        self.epoch += 1
        self._stream.wait_stream(torch.cuda.current_stream(self.device))      # (a store packed just now is finished first)
        ahead = deque()

        def enqueue(j: int) -> None:
            with torch.cuda.stream(self._stream):
                batch = self.resident.batch(batches[j], transpose=shifts[j])
                ev = torch.cuda.Event()
                ev.record(self._stream)
            ahead.append((batch, ev))

        for j in range(min(self.prefetch, len(batches))):
            enqueue(j)
        for j in range(len(batches)):
            batch, ev = ahead.popleft()
            if j + self.prefetch < len(batches):
                enqueue(j + self.prefetch)
            torch.cuda.current_stream(self.device).wait_event(ev)
            for v in batch.__dict__.values():
                if torch.is_tensor(v) and v.is_cuda:
                    v.record_stream(torch.cuda.current_stream(self.device))
            yield batch
