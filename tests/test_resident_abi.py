"""Checks of the resident data set that need no GPU: pm_dataset_pack_count, pm_dataset_pack_rows and pm_dataset_gather are
declared in include/polyphemus_hip.h ("Resident data set", directly behind "device-side graph construction" and in front of
"sampled generation"), exported by the library and bound in the ctypes table with the header's argument lists, the ABI version
is unchanged, every argument check answers PM_E_INVALID on the host before any launch (so host integers can stand in for
device addresses), the Python surface (`ops.dataset_pack`, `ops.dataset_gather`, `ops.graph_build(sizes=)`, `ResidentDataset`,
`ResidentLoader`) rejects bad arguments without a device, and the index helper the two loaders share gives the permutations
and shards the `DeviceLoader` tests expect."""
import re

import numpy as np
import pytest
import torch

from polyphemus_amd import _lib
from polyphemus_amd.data import DeviceLoader, ResidentDataset, ResidentLoader, index_batches, n_batches, shard_len
from test_abi import HEADER, header_prototypes
from test_stats_abi import _ids

SIGS = {"pm_dataset_pack_count": "pplipppps", "pm_dataset_pack_rows": "pppliplls", "pm_dataset_gather": "ppplilpppilppps"}
PM_E_INVALID = -1
# fake device addresses, 16-byte aligned and 16 MiB apart
(GRID, SGRID, BITS, CELLS, LAST, STATUS, OFF, ROWS, CPTR, INDEX, OPTR, SHIFT, S_OUT, TOK) = (0x10000000 + k * 0x1000000 for k in range(14))
n, NB, R, B, N = 5, 2, 300, 3, 200
GOOD_C = dict(token_grid=GRID, s_grid=SGRID, n=n, n_bars=NB, s_bits=BITS, cells=CELLS, last_slot=LAST, status=STATUS)
GOOD_R = dict(token_grid=GRID, s_bits=BITS, cell_off=OFF, n=n, n_bars=NB, rows=ROWS, row_base=10, R=R)
GOOD_G = dict(s_bits=BITS, rows=ROWS, cell_ptr=CPTR, n=n, n_bars=NB, R=R, index=INDEX, out_ptr=OPTR, transpose=SHIFT, B=B, N=N,
              s_tensor=S_OUT, tokens=TOK, status=STATUS)
# bytes of every buffer
BYTES_C = dict(token_grid=n * NB * 128 * 64, s_grid=n * NB * 128, s_bits=n * NB * 16, cells=4 * n, last_slot=4 * n, status=4)
BYTES_R = dict(token_grid=n * NB * 128 * 64, s_bits=n * NB * 16, cell_off=8 * (n + 1), rows=32 * R)
BYTES_G = dict(s_bits=n * NB * 16, rows=32 * R, cell_ptr=8 * (n + 1), index=4 * B, out_ptr=4 * (B + 1), transpose=4 * B,
               s_tensor=B * NB * 512, tokens=128 * N, status=8)
ALIGN = dict(token_grid=16, s_grid=1, s_bits=4, cells=4, last_slot=4, status=4, cell_off=8, rows=16, cell_ptr=8, index=4, out_ptr=4,
             transpose=4, s_tensor=16, tokens=16)


def _call(name, good, **kw):
    return getattr(_lib.lib(), name)(*{**good, **kw}.values(), None)


def _overlaps(good, nbytes, outputs):
    """every written buffer put on the first and on the last aligned piece of every other buffer, and every other buffer on
    the last piece of it"""
    bad = []
    for name in outputs:
        a = 16
        for other, size in nbytes.items():
            if other != name:
                bad += [{name: good[other]}, {name: good[other] + (size - 1) // a * a}]
                bad += [{other: good[name] + (nbytes[name] - 1) // a * a}]
    return bad


def _misaligned(good, nbytes):
    return [{name: good[name] + ALIGN[name] // 2} for name in nbytes if ALIGN[name] > 1]


def test_entries_declared_exported_and_bound():
    protos = header_prototypes()
    L = _lib.lib()
    for name, sig in SIGS.items():
        assert protos.get(name) == sig, (name, protos.get(name))
        assert hasattr(L, name), f"{name} not exported"
        assert _lib._SIGS.get(name) == sig and len(getattr(L, name).argtypes) == len(sig) and name in _lib.EXPORTED
    src = open(HEADER).read()
    titles = re.findall(r"/\* -{20,} ([^\n*]+)", src)
    at = titles.index("Resident data set")
    assert titles[at - 1] == "device-side graph construction" and titles[at + 1] == "sampled generation"
    assert (src.index("------ Resident data set") < src.index("int pm_dataset_pack_count") < src.index("int pm_dataset_pack_rows")
            < src.index("int pm_dataset_gather") < src.index("------ sampled generation"))
    section = src[src.index("------ Resident data set"):src.index("------ sampled generation")]
    assert "data.py:218-233" in section and "preprocess.py:196-205" in section
    assert int(re.search(r"#define PM_ABI_VERSION (\d+)", src).group(1)) == 9 == _lib.ABI_VERSION == L.pm_abi_version()


BIG = 1 << 31
BAD_C = ([{k: None} for k in BYTES_C] + [dict(n=0), dict(n=-1), dict(n_bars=0), dict(n_bars=-1), dict(n_bars=65), dict(n_bars=1 << 20),
                                         dict(n=BIG // (128 * NB) + 1), dict(n=1 << 62), dict(n=BIG // (128 * 64) + 1, n_bars=64)]
         + _misaligned(GOOD_C, BYTES_C) + _overlaps(GOOD_C, BYTES_C, ("s_bits", "cells", "last_slot", "status")))
BAD_R = ([{k: None} for k in BYTES_R] + [dict(n=0), dict(n=-1), dict(n_bars=0), dict(n_bars=65), dict(n=BIG // (128 * NB) + 1), dict(n=1 << 62),
                                         dict(row_base=-1), dict(row_base=R), dict(row_base=R + 5), dict(R=0), dict(R=-1, row_base=0),
                                         dict(R=(1 << 40) + 1), dict(R=1 << 62), dict(row_base=1 << 62)]
         + _misaligned(GOOD_R, BYTES_R) + _overlaps(GOOD_R, BYTES_R, ("rows",)))
BAD_G = ([{k: None} for k in BYTES_G if k != "transpose"]
         + [dict(n=0), dict(n=-1), dict(n=BIG), dict(n=1 << 62), dict(n_bars=0), dict(n_bars=-1), dict(n_bars=65), dict(R=0), dict(R=-1),
            dict(R=(1 << 40) + 1), dict(R=1 << 62), dict(B=0), dict(B=-1), dict(B=BIG // (128 * NB) + 1), dict(B=BIG - 1), dict(N=0),
            dict(N=-1), dict(N=128 * NB * B + 1), dict(N=BIG), dict(N=1 << 62), dict(N=BIG, B=BIG // (128 * NB))]
         + _misaligned(GOOD_G, BYTES_G) + _overlaps(GOOD_G, BYTES_G, ("s_tensor", "tokens", "status")))


@pytest.mark.parametrize("bad", BAD_C, ids=_ids)
def test_pack_count_rejects_on_the_host(bad):
    assert _call("pm_dataset_pack_count", GOOD_C, **bad) == PM_E_INVALID


@pytest.mark.parametrize("bad", BAD_R, ids=_ids)
def test_pack_rows_rejects_on_the_host(bad):
    assert _call("pm_dataset_pack_rows", GOOD_R, **bad) == PM_E_INVALID


@pytest.mark.parametrize("bad", BAD_G, ids=_ids)
def test_gather_rejects_on_the_host(bad):
    assert _call("pm_dataset_gather", GOOD_G, **bad) == PM_E_INVALID


def test_a_null_transpose_still_checks_everything_else():
    for bad in (dict(status=None), dict(B=0), dict(tokens=TOK + 8), dict(s_tensor=ROWS), dict(N=128 * NB * B + 1)):
        assert _call("pm_dataset_gather", GOOD_G, transpose=None, **bad) == PM_E_INVALID


def _cpu_store(n=4, nb=2):
    """a store on the CPU, built by hand: sample i has its first i + 1 steps of track 1 active in bar 0 and cell [0,0] in bar 1"""
    bits = torch.zeros(n, nb, 4, dtype=torch.int32)
    for i in range(n):
        bits[i, 0, 1] = (1 << (i + 1)) - 1
        bits[i, 1:, 0] = 1
    nodes = np.array([i + 1 + (nb - 1) for i in range(n)], np.int32)
    ptr = np.zeros(n + 1, np.int64)
    np.cumsum(nodes, out=ptr[1:])
    rows = torch.zeros(int(ptr[-1]), 16, 2, dtype=torch.uint8)
    edges = np.array([max(2 * i, 1) + (nb - 1) for i in range(n)], np.int32)
    return dict(s_bits=bits, rows=rows, cell_ptr=torch.from_numpy(ptr), nodes=nodes, edges=edges, last_slot=np.ones(n, np.int32), n_bars=nb)


def test_python_surface_rejects_bad_arguments_without_a_device():
    from polyphemus_amd import ops
    a = _cpu_store()
    ds = ResidentDataset(**a)
    assert len(ds) == 4 and ds.n_bars == 2 and ds.nbytes == 4 * 2 * 16 + 32 * 14 + 8 * 5

    # the constructor
    for kw, name in ([(dict(s_bits=v), "s_bits") for v in (a["s_bits"].long(), a["s_bits"][:, :1], a["s_bits"].reshape(-1), a["s_bits"].numpy(), a["s_bits"][:0])]
                     + [(dict(rows=v), "rows") for v in (a["rows"].int(), a["rows"][:, :15], a["rows"].reshape(-1), None, a["rows"][:0])]
                     + [(dict(cell_ptr=v), "cell_ptr") for v in (a["cell_ptr"].int(), a["cell_ptr"][:-1], a["cell_ptr"].tolist())]
                     + [(dict(n_bars=v), "n_bars") for v in (0, -1, 2.0, True, None, 65)]
                     + [(dict(nodes=v), "nodes") for v in (a["nodes"][:-1], a["nodes"].astype(np.float32), a["nodes"] + 1, a["nodes"] * 0)]
                     + [(dict(edges=v), "edges") for v in (a["edges"][:-1], a["edges"] * 0, a["edges"].astype(np.float64))]
                     + [(dict(last_slot=v), "last_slot") for v in (a["last_slot"][:-1], a["last_slot"] + 15, a["last_slot"] - 2)]):
        with pytest.raises(ValueError, match=name):
            ResidentDataset(**{**a, **kw})

    # batch: the index and the shifts are checked on the host, before the device is asked for
    for bad in ([], [4], [-1], [0, 1, 4], [0.5], [True], "01", None, 3, np.zeros((1, 2), np.int64), np.zeros(2), torch.zeros(2),
                torch.tensor([0, 5]), np.array([1 << 40])):
        with pytest.raises(ValueError, match="index"):
            ds.batch(bad)
    for bad in ([128, 0], [0, -128], [1], [1, 2, 3], [0.5, 1.0], np.zeros(2), torch.zeros(2), np.zeros((2, 1), np.int32), "random", 5):
        with pytest.raises(ValueError, match="transpose"):
            ds.batch([0, 1], transpose=bad)
    for index, kw in (([0, 1], {}), (np.array([3, 3, 0]), dict(transpose=[127, -127, 0])), (torch.tensor([2]), dict(check=True)),
                      (range(4), dict(transpose=np.array([-5, 6, 0, 1], np.int64)))):
        with pytest.raises(_lib.HipExtensionError, match="no CPU fallback"):
            ds.batch(index, **kw)

    # ops.dataset_gather
    idx, optr = torch.tensor([0, 1], dtype=torch.int32), torch.tensor([0, 2, 5], dtype=torch.int32)
    gather = lambda **kw: ops.dataset_gather(**{**dict(s_bits=a["s_bits"], rows=a["rows"], cell_ptr=a["cell_ptr"], n_bars=2, index=idx,
                                                       out_ptr=optr, N=5), **kw})
    for kw, name in ([(dict(s_bits=v), "s_bits") for v in (a["s_bits"].long(), a["s_bits"][:, :1], None)]
                     + [(dict(rows=v), "rows") for v in (a["rows"].int(), a["rows"][:, :15], a["rows"].numpy())]
                     + [(dict(cell_ptr=v), "cell_ptr") for v in (a["cell_ptr"].int(), a["cell_ptr"][:-1])]
                     + [(dict(n_bars=v), "n_bars") for v in (0, 2.0, True, 65)]
                     + [(dict(index=v), "index") for v in (idx.long(), idx[:0], idx.view(1, -1), [0, 1], None)]
                     + [(dict(out_ptr=v), "out_ptr") for v in (optr.long(), optr[:2], [0, 2, 5], None)]
                     + [(dict(transpose=v), "transpose") for v in (torch.zeros(2), torch.zeros(3, dtype=torch.int32), [0, 0], 1)]
                     + [(dict(N=v), "N") for v in (0, -1, 5.0, True, None, 128 * 2 * 2 + 1)]):
        with pytest.raises(ValueError, match=name):
            gather(**kw)
    for kw in (dict(), dict(transpose=torch.zeros(2, dtype=torch.int32))):
        with pytest.raises(_lib.HipExtensionError, match="no CPU fallback"):
            gather(**kw)

    # ops.dataset_pack
    tok, s = torch.zeros(3, 2, 4, 32, 16, 2, dtype=torch.int16), torch.zeros(3, 2, 4, 32, dtype=torch.uint8)
    for kw, name in ([(dict(token_grid=v), "token_grid") for v in (tok.int(), tok[..., :1], tok[:0], tok.numpy(), tok.reshape(3, -1),
                                                                    torch.zeros(1, 65, 4, 32, 16, 2, dtype=torch.int16))]
                     + [(dict(s_grid=v), "s_grid") for v in (s.bool(), s[:2], s.float(), s.numpy(), s.reshape(3, -1))]
                     + [(dict(rows=v), "rows") for v in (a["rows"].int(), a["rows"][:, :15], a["rows"].numpy())]
                     + [(dict(row_base=v), "row_base") for v in (-1, 1, 2.0, True, None)]
                     + [(dict(rows=a["rows"], row_base=15), "row_base")]):
        with pytest.raises(ValueError, match=name):
            ops.dataset_pack(**{**dict(token_grid=tok, s_grid=s), **kw})
    for kw in (dict(), dict(rows=a["rows"], row_base=14)):
        with pytest.raises(_lib.HipExtensionError, match="no CPU fallback"):
            ops.dataset_pack(tok, s, **kw)

    # ops.graph_build(sizes=)
    for bad in ((1,), (0, 1), (1, 0), (1.0, 2), [1, 2, 3], 5, (1 << 31, 1), (True, 1)):
        with pytest.raises(ValueError, match="sizes"):
            ops.graph_build(torch.zeros(2, 4, 32), 2, sizes=bad)
    with pytest.raises(_lib.HipExtensionError, match="no CPU fallback"):
        ops.graph_build(torch.zeros(2, 4, 32), 2, sizes=(2, 2))

    # the constructors and the loader
    for kw, name in ((dict(token_grid=tok.int()), "token_grid"), (dict(token_grid=tok[..., :1]), "token_grid"), (dict(s_grid=s[:2]), "s_grid"),
                     (dict(s_grid=s.float()), "s_grid"), (dict(chunk=0), "chunk"), (dict(chunk=2.0), "chunk"), (dict(chunk=True), "chunk")):
        with pytest.raises(ValueError, match=name):
            ResidentDataset.from_arrays(**{**dict(token_grid=tok, s_grid=s, device="cpu"), **kw})
    with pytest.raises(_lib.HipExtensionError, match="no CPU fallback"):
        ResidentDataset.from_arrays(tok.numpy(), s.numpy().astype(bool), device="cpu")
    for kw, name in ((dict(resident=None), "resident"), (dict(batch_size=0), "batch_size"), (dict(batch_size=2.0), "batch_size"),
                     (dict(transpose="up"), "transpose"), (dict(transpose=3), "transpose"), (dict(prefetch=0), "prefetch"),
                     (dict(prefetch=True), "prefetch"), (dict(rank=2, world=2), "rank")):
        with pytest.raises(ValueError, match=name):
            ResidentLoader(**{**dict(resident=ds, batch_size=2), **kw})
    loader = ResidentLoader(ds, batch_size=3, rank=0, world=1)
    assert len(loader) == 2 and loader.n_bars == 2
    with pytest.raises(_lib.HipExtensionError, match="no CPU fallback"):
        next(iter(loader))


def test_load_rejects_a_file_that_is_no_store(tmp_path):
    np.savez(tmp_path / "x.npz", rows=np.zeros((1, 16, 2), np.uint8))
    with pytest.raises(ValueError, match="not a resident data set"):
        ResidentDataset.load(str(tmp_path / "x.npz"), device="cpu")
    a = _cpu_store()
    np.savez(tmp_path / "y.npz", s_bits=a["s_bits"].numpy().view(np.uint32), rows=a["rows"].numpy(), cell_ptr=a["cell_ptr"].numpy() + 1,
             nodes=a["nodes"], edges=a["edges"], last_slot=a["last_slot"], n_bars=np.int32(2))
    with pytest.raises(ValueError, match="do not agree"):
        ResidentDataset.load(str(tmp_path / "y.npz"), device="cpu")


def _plan(cls, n, bs, shuffle, seed, epoch, drop_last, rank, world):
    """the index plan of a loader made without its device half (as tests/test_parallel_cpu.py makes `DeviceLoader`'s)"""
    class Sized:
        n_bars = 2

        def __len__(self):
            return n
    ld = cls.__new__(cls)
    ld.dataset = ld.resident = Sized()
    ld.batch_size, ld.shuffle, ld.seed, ld.drop_last, ld.epoch, ld.rank, ld.world = bs, shuffle, seed, drop_last, epoch, rank, world
    return ld._index_batches(), len(ld)


def test_the_shared_index_helper_gives_the_plans_the_device_loader_tests_expect():
    # tests/test_data_gpu.py: plain order with the partial last batch, drop_last, shuffle with seed 7 over two epochs
    plain = index_batches(11, 4, False, 0, 0, False, 0, 1)
    assert [list(b) for b in plain] == [[0, 1, 2, 3], [4, 5, 6, 7], [8, 9, 10]] and n_batches(11, 4, False, 1) == 3
    assert [list(b) for b in index_batches(11, 4, False, 0, 0, True, 0, 1)] == [[0, 1, 2, 3], [4, 5, 6, 7]] and n_batches(11, 4, True, 1) == 2
    for epoch in (0, 1):
        order = np.random.default_rng(7 + epoch).permutation(11)
        got = index_batches(11, 4, True, 7, epoch, False, 0, 1)
        assert [list(b) for b in got] == [list(order[4 * j:4 * j + 4]) for j in range(3)]
    # tests/test_parallel_cpu.py: world 2 at epoch 3, one wrapped duplicate
    order = np.random.default_rng(5 + 3).permutation(11)
    plans = [index_batches(11, 2, True, 5, 3, False, rank, 2) for rank in range(2)]
    assert all(len(p) == n_batches(11, 2, False, 2) == 3 for p in plans) and shard_len(11, 2) == 6
    assert list(np.concatenate(plans[0])) == list(np.concatenate([order, order[:1]])[0::2])
    assert list(np.concatenate(plans[1])) == list(np.concatenate([order, order[:1]])[1::2])
    # ... world 8, a data set smaller than the world included: lock step, every sample covered
    for n_, world, bs in ((2051, 8, 256), (5, 8, 2), (8, 8, 1), (17, 8, 4)):
        plans = [index_batches(n_, bs, True, 11, 0, False, rank, world) for rank in range(world)]
        assert len({len(p) for p in plans}) == 1 and len(plans[0]) == n_batches(n_, bs, False, world)
        assert all(sum(len(b) for b in p) == -(-n_ // world) for p in plans)
        assert set(np.concatenate([np.concatenate(p) for p in plans])) == set(range(n_))
    # both loaders go through the helper: equal plans and lengths for equal arguments
    for args in ((11, 4, False, 0, 0, False, 0, 1), (11, 4, True, 7, 1, True, 0, 1), (11, 2, True, 5, 3, False, 1, 2), (11, 2, False, 0, 0, False, 2, 3),
                 (5, 2, True, 11, 2, False, 6, 8)):
        want, dev, res = index_batches(*args), _plan(DeviceLoader, *args), _plan(ResidentLoader, *args)
        assert dev[1] == res[1] == len(want) == n_batches(args[0], args[1], args[5], args[7])
        assert [list(b) for b in dev[0]] == [list(b) for b in res[0]] == [list(b) for b in want]


def test_random_shifts_are_drawn_per_sample_epoch_and_rank():
    ds = ResidentDataset(**_cpu_store())
    draws = {}
    for seed, epoch, rank in ((3, 0, 0), (3, 1, 0), (3, 0, 1), (4, 0, 0)):
        ld = ResidentLoader(ds, batch_size=3, shuffle=True, seed=seed, transpose="random", rank=rank, world=2)
        ld.epoch = epoch
        batches = ld._index_batches()
        shifts = ld._shifts(batches)
        assert [len(s) for s in shifts] == [len(b) for b in batches] and all(s.dtype == np.int32 and -5 <= s.min() and s.max() <= 6 for s in shifts)
        want = np.random.default_rng([seed, epoch, rank]).integers(-5, 7, size=sum(len(b) for b in batches))
        assert list(np.concatenate(shifts)) == list(want)
        draws[(seed, epoch, rank)] = list(want)
    assert ResidentLoader(ds, batch_size=3, rank=0, world=1)._shifts([np.arange(3)]) == [None]
