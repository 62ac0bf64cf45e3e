"""The resident data set (polyphemus_amd/data.py `ResidentDataset` / `ResidentLoader`, csrc/dataset.hip) against the host
construction (`collate_samples` of `sample_from_disk`), `collate_on_device`, `DeviceLoader` and the batch the reference's own
DataLoader built from the golden samples: integer work, everything bit-exact.  Eleven synthetic two-bar samples, four of
them replaced by the shapes where the kernels can go wrong: an empty first bar, both bars empty (the [0,0] rule and the row the
grid holds there), a cell with 14 notes (slot 15 live, n_slots = 15) and p = 1 (256 cells, the most a sample holds)."""
import os

import numpy as np
import pytest
import torch

from polyphemus_amd import _lib, ops
from polyphemus_amd import constants as C
from polyphemus_amd.data import (DeviceLoader, PolyphemusDataset, ResidentDataset, ResidentLoader, collate_on_device,
                                 relayout_sample)
from polyphemus_amd.generate import NoteBatch
from polyphemus_amd.graphs import collate_samples
from polyphemus_amd.model import VAE
from polyphemus_amd.synthetic import disk_sample, sample_from_disk
from polyphemus_amd.trainer import HipTrainer
from test_data_gpu import KEYS, write_disk
from util import batch_from_golden, load_case

pytestmark = pytest.mark.gpu
DEV = "cuda"
EMPTY_FIRST, EMPTY_BOTH, FULL_SLOTS, FULL_CELLS = 3, 5, 7, 9
SPECIAL = (EMPTY_FIRST, EMPTY_BOTH, FULL_SLOTS, FULL_CELLS)


def make_disk(nb, count, seed):
    rng = np.random.default_rng(seed)
    return [disk_sample(rng, nb, 0.2) for _ in range(count)], rng


def special_disk():
    disk, rng = make_disk(2, 11, 5)
    disk[EMPTY_FIRST][1][:, :32] = False
    disk[EMPTY_BOTH][1][:] = False
    c, s = disk_sample(rng, 2, 0.2, max_notes=14)
    tr, ts = (int(v[0]) for v in np.nonzero(s))                       # one cell for sure with 14 notes: EOS in slot 15
    c[tr, ts, 1:15, 0], c[tr, ts, 1:15, 1] = np.arange(40, 54), 3
    c[tr, ts, 15] = (C.PITCH_EOS, C.DUR_EOS)
    disk[FULL_SLOTS] = (c, s)
    disk[FULL_CELLS] = disk_sample(rng, 2, 1.0)
    # sample 1 (at most 4 notes per cell elsewhere): its only cell with 14 notes shares its step with a one-note cell of a later
    # track, so the last live slot is not that of the step's last cell
    c, s = disk[1]
    ts = int(np.nonzero(s[0])[0][0])
    c[0, ts, 1:15, 0], c[0, ts, 1:15, 1] = np.arange(50, 64), 5
    c[0, ts, 15] = (C.PITCH_EOS, C.DUR_EOS)
    s[3, ts] = True
    c[3, ts, 1:] = (C.PITCH_PAD, C.DUR_PAD)
    c[3, ts, 1], c[3, ts, 2] = (60, 7), (C.PITCH_EOS, C.DUR_EOS)
    return disk


def transposed(c_disk, shift):
    """preprocess.py:196-205 restated: on tracks 1.. the pitches that are not SOS, EOS or PAD move by `shift`, clipped to 0..127"""
    c = c_disk.copy()
    pitch = c[1:, ..., 0].astype(np.int64)
    c[1:, ..., 0] = np.where(pitch <= 127, np.clip(pitch + int(shift), 0, 127), pitch).astype(c.dtype)
    return c


def host_batch(disk, idx, nb, shifts=None):
    shifts = [0] * len(idx) if shifts is None else shifts
    return collate_samples([sample_from_disk(transposed(disk[i][0], sh), disk[i][1].copy(), nb) for i, sh in zip(idx, shifts)], nb)


def stacked(disk, nb):
    pairs = [relayout_sample(c, s, nb) for c, s in disk]
    return np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])


def assert_same(dev, ref):
    assert dev.num_nodes == ref.num_nodes
    for k in KEYS:
        a, b = getattr(dev, k).cpu(), getattr(ref, k).cpu()
        assert a.dtype == b.dtype and a.shape == b.shape and bool((a == b).all()), k


def assert_same_as_device_collate(got, ref):
    """every key of `collate_on_device`'s batch"""
    assert_same(got, ref)
    assert (got.n_slots, got.track_unique, got.n_bars) == (ref.n_slots, ref.track_unique, ref.n_bars) and got.track_unique is True
    assert got.node_cell.dtype == ref.node_cell.dtype and torch.equal(got.node_cell, ref.node_cell)
    assert set(ref.__dict__) <= set(got.__dict__) and "transpose" in got.__dict__


def device_collate(disk, idx, nb):
    return collate_on_device([relayout_sample(disk[i][0], disk[i][1], nb) for i in idx], nb, DEV)


@pytest.fixture(scope="module")
def disk():
    return special_disk()


@pytest.fixture(scope="module")
def resident(disk):
    return ResidentDataset.from_arrays(*stacked(disk, 2), device=DEV)


@pytest.fixture(scope="module")
def on_disk(disk, tmp_path_factory):
    path = tmp_path_factory.mktemp("resident")
    write_disk(path, disk)
    return PolyphemusDataset(str(path), 2)


def test_the_store_is_what_the_issue_lays_out(disk, resident):
    assert len(resident) == 11 and resident.n_bars == 2
    assert (resident.s_bits.dtype, tuple(resident.s_bits.shape)) == (torch.int32, (11, 2, 4))
    nodes = np.array([host_batch(disk, [i], 2).num_nodes for i in range(11)])
    assert nodes[FULL_CELLS] == 256 and nodes[EMPTY_BOTH] == 2
    assert (resident.rows.dtype, tuple(resident.rows.shape)) == (torch.uint8, (int(nodes.sum()), 16, 2))
    assert resident.cell_ptr.dtype == torch.int64 and resident.cell_ptr.tolist() == [0] + list(np.cumsum(nodes))
    assert resident.nbytes == 11 * 2 * 16 + 32 * int(nodes.sum()) + 8 * 12
    assert list(resident._nodes) == list(nodes)
    assert list(resident._edges) == [host_batch(disk, [i], 2).edge_type.numel() for i in range(11)]
    assert list(resident._last) == [host_batch(disk, [i], 2).n_slots for i in range(11)]      # (every cell holds a note: >= 2)
    assert resident._last[FULL_SLOTS] == 15 and all(a.dtype == np.int32 for a in (resident._nodes, resident._edges, resident._last))
    tokens = torch.cat([host_batch(disk, [i], 2).tokens for i in range(11)])
    assert torch.equal(resident.rows.cpu().int(), tokens)


INDEX_LISTS = [list(range(11)), [10, 3, 0, 7, 5, 9, 1, 8, 2, 6, 4], [9, 9, 5, 0, 5, 3, 3, 9]] + [[i] for i in SPECIAL]


@pytest.mark.parametrize("index", INDEX_LISTS, ids=lambda v: "-".join(map(str, v)))
def test_batch_equals_the_host_truth(disk, resident, index):
    want = host_batch(disk, index, 2)
    for form in (index, np.asarray(index), torch.tensor(index), torch.tensor(index, dtype=torch.int32)):
        got = resident.batch(form, check=True)
        assert_same(got, want)
        assert got.n_slots == want.n_slots and got.transpose is None
    assert_same_as_device_collate(got, device_collate(disk, index, 2))
    if index == [FULL_SLOTS]:
        assert got.n_slots == 15
    if index == [EMPTY_BOTH]:
        assert got.num_nodes == 2 and got.tokens[:, 0].tolist() == [[C.PITCH_SOS, C.DUR_SOS]] * 2


@pytest.mark.parametrize("nb", [1, 3])
def test_other_bar_counts(nb):
    disk, _ = make_disk(nb, 5, 20 + nb)
    disk[2][1][:, :32] = False
    res = ResidentDataset.from_arrays(*stacked(disk, nb), device=DEV)
    for index in ([0, 1, 2, 3, 4], [4, 2, 2, 0]):
        got = res.batch(index, check=True)
        assert_same(got, host_batch(disk, index, nb))
        assert_same_as_device_collate(got, device_collate(disk, index, nb))


@pytest.mark.parametrize("case", ["lmd2_tiny", "nb3_tiny"])
def test_golden_samples_equal_the_reference_dataloader(case, tmp_path):
    z, cfg = load_case(case)
    nb = cfg["n_bars"]
    n = len([k for k in z.files if k.startswith("disk/") and k.endswith("/s_tensor")])
    write_disk(tmp_path, [(z[f"disk/{i}/c_tensor"], z[f"disk/{i}/s_tensor"]) for i in range(n)])
    ref = batch_from_golden(z, cfg)                                   # built by the reference (oracle/make_golden.py)
    for kw in (dict(), dict(chunk=1, num_workers=2)):
        res = ResidentDataset.from_dataset(PolyphemusDataset(str(tmp_path), nb), device=DEV, **kw)
        assert len(res) == n and res.n_bars == nb
        got = res.batch(range(n), check=True)
        assert_same(got, ref)
        assert (got.n_slots, got.track_unique) == (ref.n_slots, ref.track_unique)
    assert_same(next(iter(ResidentLoader(res, batch_size=n))), ref)


def test_chunking_does_not_show(disk, resident, on_disk):
    tok, s = stacked(disk, 2)
    for chunk in (4, 1024, 1, 11):
        assert ResidentDataset.from_arrays(tok, s, device=DEV, chunk=chunk) == resident, chunk
    assert ResidentDataset.from_arrays(torch.from_numpy(tok), torch.from_numpy(s).bool(), device=DEV, chunk=3) == resident
    assert ResidentDataset.from_dataset(on_disk, device=DEV, chunk=4) == ResidentDataset.from_dataset(on_disk, device=DEV, chunk=1024) == resident
    assert ResidentDataset.from_dataset(on_disk, device=DEV, chunk=5, num_workers=3) == resident
    other = ResidentDataset.from_arrays(tok[:10], s[:10], device=DEV)
    assert other != resident and len(other) == 10


def test_save_and_load_give_the_same_store_and_batches(disk, resident, tmp_path):
    path = str(tmp_path / "store.npz")
    resident.save(path)
    with np.load(path) as z:
        assert z["s_bits"].dtype == np.uint32 and z["rows"].dtype == np.uint8 and z["cell_ptr"].dtype == np.int64
        assert all(z[k].dtype == np.int32 and z[k].shape == (11,) for k in ("nodes", "edges", "last_slot")) and int(z["n_bars"]) == 2
        arrays = {k: z[k] for k in z.files}
    back = ResidentDataset.load(path, device=DEV)
    assert back == resident and back.nbytes == resident.nbytes
    index = [9, 0, 5, 5, 7]
    assert_same_as_device_collate(back.batch(index, check=True), resident.batch(index))
    assert_same(back.batch(index), host_batch(disk, index, 2))
    arrays["edges"] = arrays["edges"].copy()
    arrays["edges"][4] += 1                                           # counts that nobody reads back later are checked here
    np.savez(path, **arrays)
    with pytest.raises(ValueError, match="edges do not agree"):
        ResidentDataset.load(path, device=DEV)


def test_a_token_id_out_of_range_raises_at_pack_time(disk):
    tok, s = stacked(disk, 2)
    b, k, t = (int(v[0]) for v in np.nonzero(s[2]))
    bad = tok.copy()
    bad[2, b, k, t, 3, 0] = 131
    with pytest.raises(ValueError, match="1 token ids"):
        ResidentDataset.from_arrays(bad, s, device=DEV)
    bad[2, b, k, t, 9, 1], bad[6, 1, 0, 0, 0, 0] = 99, -1             # sample 6, bar 1, cell [0,0]: active or not, see below
    count = 2 + int(s[6, 1, 0, 0] != 0)
    with pytest.raises(ValueError, match=f"{count} token ids"):
        ResidentDataset.from_arrays(bad, s, device=DEV, chunk=4)
    quiet = tok.copy()
    bi, ki, ti = (int(v[0]) for v in np.nonzero(s[2] == 0))
    quiet[2, bi, ki, ti, 1] = (131, 99)                               # an inactive cell is never read
    assert ResidentDataset.from_arrays(quiet, s, device=DEV) == ResidentDataset.from_arrays(tok, s, device=DEV)


def assert_loaders_agree(res_loader, dev_loader, epochs=1):
    for _ in range(epochs):
        got, want = list(res_loader), list(dev_loader)
        assert len(got) == len(want) == len(res_loader) == len(dev_loader) and len(got) > 0
        for a, b in zip(got, want):
            assert_same_as_device_collate(a, b)
    return got


def test_resident_loader_equals_device_loader(disk, resident, on_disk):
    got = assert_loaders_agree(ResidentLoader(resident, batch_size=4), DeviceLoader(on_disk, batch_size=4, device=DEV))
    assert [b.s_tensor.shape[0] for b in got] == [8, 8, 6]
    assert_same(got[2], host_batch(disk, [8, 9, 10], 2))
    got = assert_loaders_agree(ResidentLoader(resident, batch_size=11, prefetch=1), DeviceLoader(on_disk, batch_size=11, device=DEV))
    assert len(got) == 1
    got = assert_loaders_agree(ResidentLoader(resident, batch_size=4, drop_last=True), DeviceLoader(on_disk, batch_size=4, device=DEV, drop_last=True))
    assert len(got) == 2
    assert_loaders_agree(ResidentLoader(resident, batch_size=4, shuffle=True, seed=7, prefetch=3),
                         DeviceLoader(on_disk, batch_size=4, shuffle=True, seed=7, device=DEV), epochs=2)
    order2 = np.random.default_rng(8).permutation(11)
    sh = ResidentLoader(resident, batch_size=4, shuffle=True, seed=7)
    list(sh)
    assert_same(next(iter(sh)), host_batch(disk, order2[:4], 2))
    for rank in range(3):                                             # 11 samples over 3 ranks: wrap-around repeats one
        got = assert_loaders_agree(ResidentLoader(resident, batch_size=2, shuffle=True, seed=1, rank=rank, world=3),
                                   DeviceLoader(on_disk, batch_size=2, shuffle=True, seed=1, device=DEV, rank=rank, world=3))
        assert sum(b.s_tensor.shape[0] for b in got) == 2 * 4


SHIFTS = [-5, 6, 0, 127, -127, 3, -12, 1, 5, -1, 2]


def test_explicit_transposition_equals_the_restated_rule(disk, resident):
    index = list(range(11))
    plain = resident.batch(index)
    for shifts in (SHIFTS, np.asarray(SHIFTS, np.int64), torch.tensor(SHIFTS, dtype=torch.int32)):
        got = resident.batch(index, transpose=shifts, check=True)
        assert_same(got, host_batch(disk, index, 2, SHIFTS))
        assert got.transpose.dtype == torch.int32 and got.transpose.tolist() == SHIFTS and got.n_slots == plain.n_slots
    tok, was = got.tokens.cpu(), plain.tokens.cpu()
    drum, sample = plain.is_drum.cpu(), plain.batch.cpu()
    assert torch.equal(tok[drum], was[drum]) and torch.equal(tok[..., 1], was[..., 1])                # drums, durations
    marks = was[..., 0] > 127
    assert bool(marks.any()) and torch.equal(tok[..., 0][marks], was[..., 0][marks])                   # SOS, EOS, PAD
    moved = ~marks & ~drum[:, None]
    for i, sh in enumerate(SHIFTS):
        m = moved & (sample == i)[:, None]
        assert bool(m.any()) == (i != EMPTY_BOTH) and torch.equal(tok[..., 0][m], (was[..., 0][m] + sh).clamp(0, 127))
    assert set(tok[..., 0][moved & (sample == 3)[:, None]].tolist()) == {127} and set(tok[..., 0][moved & (sample == 4)[:, None]].tolist()) == {0}
    # a permutation with repeats, each entry under its own shift
    index, shifts = [9, 5, 9, 3, 7], [12, -3, -12, 127, -40]
    assert_same(resident.batch(index, transpose=shifts, check=True), host_batch(disk, index, 2, shifts))
    assert_same(resident.batch(index, transpose=[0] * 5), host_batch(disk, index, 2))


def test_random_transposition(disk, resident):
    make = lambda seed: ResidentLoader(resident, batch_size=4, shuffle=True, seed=seed, transpose="random")
    a, b = make(3), make(3)
    epochs = []
    for epoch in range(2):
        order = np.random.default_rng(3 + epoch).permutation(11)
        drawn = []
        for j, (x, y) in enumerate(zip(a, b)):
            shifts = x.transpose.tolist()
            assert all(-5 <= v <= 6 for v in shifts) and shifts == y.transpose.tolist() and len(shifts) == x.s_tensor.shape[0] // 2
            assert_same(x, y)
            assert_same(x, host_batch(disk, order[4 * j:4 * j + 4], 2, shifts))
            drawn += shifts
        assert len(drawn) == 11
        epochs.append(drawn)
    assert epochs[0] != epochs[1]
    assert epochs[0] == list(np.random.default_rng([3, 0, 0]).integers(-5, 7, size=11))
    assert [v for x in make(4) for v in x.transpose.tolist()] != epochs[0]
    assert all(x.transpose is None for x in ResidentLoader(resident, batch_size=4))


def test_a_batch_costs_no_host_read(disk, resident):
    index = [4, 9, 0, 5]
    loader = ResidentLoader(resident, batch_size=4, shuffle=True, seed=2, transpose="random")
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = resident.batch(index)
        shifted = resident.batch(index, transpose=[1, -1, 0, 6])
        epoch = list(loader)
        with pytest.raises(RuntimeError, match="synchroniz"):         # the mode was live: `check` is the one host read
            resident.batch(index, check=True)
    finally:
        torch.cuda.set_sync_debug_mode(before)
    assert_same(got, host_batch(disk, index, 2))
    assert_same(shifted, host_batch(disk, index, 2, [1, -1, 0, 6]))
    order = np.random.default_rng(2).permutation(11)
    assert len(epoch) == 3
    for j, b in enumerate(epoch):
        assert_same(b, host_batch(disk, order[4 * j:4 * j + 4], 2, b.transpose.tolist()))


def test_the_gather_counts_what_it_does_not_follow(disk, resident):
    n = len(resident)
    nodes = resident._nodes
    good_index, bad_index = [2, 9, 0, 4, 6], [2, 9, n, 4, 6]          # entry 2: an index equal to n, given sample 0's span
    out_ptr = np.concatenate([[0], np.cumsum(nodes[good_index])]).astype(np.int32)
    N = int(out_ptr[-1])
    short = out_ptr.copy()
    short[-1] -= 1                                                    # entry 4: a span one row short
    dev = lambda a: torch.tensor(np.asarray(a), dtype=torch.int32, device=DEV)
    gather = lambda index, ptr: ops.dataset_gather(resident.s_bits, resident.rows, resident.cell_ptr, 2, dev(index), dev(ptr), N)
    s0, tok0, status0 = gather(good_index, out_ptr)
    assert status0.tolist() == [0, 0]
    want = host_batch(disk, good_index, 2)
    assert torch.equal(tok0.cpu(), want.tokens) and torch.equal(s0.cpu(), want.s_tensor)
    s1, tok1, status1 = gather(bad_index, short)
    assert status1.tolist() == [1, 1]
    for j in (0, 1, 3):                                               # the entries that were followed: as in the clean call
        assert torch.equal(tok1[out_ptr[j]:out_ptr[j + 1]], tok0[out_ptr[j]:out_ptr[j + 1]]), j
        assert torch.equal(s1[2 * j:2 * j + 2], s0[2 * j:2 * j + 2]), j
    for j in (2, 4):                                                  # the others: a structure of zeros
        assert not bool(s1[2 * j:2 * j + 2].any()), j
    # rows an entry was not given stay as they were: the same call into buffers of a known value is not possible through
    # ops (it allocates), so the span one row short is checked through its neighbour instead: entry 3 is intact up to its end
    assert torch.equal(tok1[out_ptr[4] - 1], tok0[out_ptr[4] - 1])
    with pytest.raises(ValueError, match="index: 1 entries outside"):
        resident.batch(bad_index)


def test_from_notes_equals_the_note_batch_as_a_graph():
    chord = [(40, 30 + j, 2 + j) for j in range(16)]                  # 16 notes on one step: 14 are kept, EOS lands in slot 15
    pieces = [[[(0, 36, 4), (8, 38, 2), (40, 36, 4)], [(0, 40, 8), (33, 43, 8)], [(4, 60, 2), (4, 64, 2), (50, 62, 6)], [(16, 72, 16), (60, 70, 4)]],
              [[(3, 36, 1)], [], [(5, 55, 3), (31, 57, 96)], []],                                   # bar 1 silent in every track
              [[(1, 42, 1)], chord, [(63, 50, 1)], [(40, 77, 5)]]]
    nb = NoteBatch.from_lists(pieces, 2, device=DEV)
    want = nb.to_graph()
    for chunk in (1024, 1, 2):
        res = ResidentDataset.from_notes(nb, chunk=chunk)
        assert len(res) == 3 and res.n_bars == 2 and list(res._last) == [3, 2, 15]     # two notes on a step, one, fourteen (+ EOS)
        got = res.batch(range(3), check=True)
        assert_same_as_device_collate(got, want)
    assert got.n_slots == 15 and int(got.s_tensor[3].sum()) == 1 and float(got.s_tensor[3, 0, 0]) == 1.0


def test_training_from_the_resident_loader_equals_training_from_the_device_loader(resident, on_disk):
    """the two loaders deliver the same bits, so in deterministic mode two steps give the same bits"""
    cfg = dict(dropout=0, batch_norm=True, gnn_n_layers=2, d=32, n_bars=2, resolution=8)
    epss = [torch.randn(4, 32, generator=torch.Generator().manual_seed(i)).to(DEV) for i in range(2)]
    faults0 = _lib.deterministic_faults()
    out = []
    with _lib.deterministic(True):
        for use_resident in (True, False):
            torch.manual_seed(0)
            vae = VAE(**cfg, device=DEV).to(DEV)
            vae.train()
            tr = HipTrainer(vae, lr=1e-4)
            batches = ResidentLoader(resident, batch_size=4, drop_last=True) if use_resident else \
                DeviceLoader(on_disk, batch_size=4, device=DEV, drop_last=True)
            losses = [tr.train_step(b, e).clone() for b, e in zip(batches, epss)]
            assert len(losses) == 2
            out.append((losses, vae.flat_params.clone()))
        torch.cuda.synchronize()
        assert _lib.deterministic_faults() == faults0
    (la, pa), (lb, pb) = out
    for x, y in zip(la, lb):
        assert torch.isfinite(x).all() and torch.equal(x, y)
    assert torch.equal(pa, pb)
