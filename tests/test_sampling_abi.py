"""Checks of sampled generation that need no GPU: its three entries are declared in include/polyphemus_hip.h, exported by
the library and bound in the ctypes table with the header's argument lists, the ABI version is unchanged, every argument
check answers PM_E_INVALID on the host before any launch (so host integers can stand in for device addresses), the noise
stream's host entry equals its numpy restatement and is uniform, and `generate_music` rejects bad sampling arguments before
it touches the model."""
import ctypes
import re

import numpy as np
import pytest

from polyphemus_amd import _lib
from test_abi import HEADER, header_prototypes
from util import _mix32

ENTRIES = {"pm_sample_tokens": "plfifups", "pm_mtp_from_tokens": "ppilppps"}
PM_E_INVALID = -1
# fake device addresses, 16-byte aligned and 1 MiB apart
LOGITS, TOKENS, S, BARS, PTR, MTP = (0x10000000 + k * 0x100000 for k in range(6))
_M32 = np.uint64(0xFFFFFFFF)


def sample_hash_np(seed, row, head, token):
    """h >> 9 of the header's draw, for uint64 arrays (or ints) holding 32-bit values: the 23 bits u is made of."""
    seed, row, head, token = (np.asarray(a, dtype=np.uint64) for a in (seed, row, head, token))
    k0 = _mix32(seed ^ (((head + np.uint64(1)) * np.uint64(0x9E3779B9)) & _M32))
    key = _mix32(k0 ^ ((row * np.uint64(0x85EBCA6B) + np.uint64(0x27D4EB2F)) & _M32))
    return _mix32((key + token * np.uint64(0xC2B2AE35)) & _M32) >> np.uint64(9)


def _sample(c_logits=LOGITS, rows=15, temperature=1.0, top_k=0, top_p=1.0, seed=0, tokens=TOKENS):
    return _lib.lib().pm_sample_tokens(c_logits, rows, temperature, top_k, top_p, seed, tokens, None)


def _mtp(tokens=TOKENS, s=S, G=2, N=7, bars=BARS, ptr=PTR, mtp=MTP):
    return _lib.lib().pm_mtp_from_tokens(tokens, s, G, N, bars, ptr, mtp, None)


def test_sampling_entries_declared_exported_and_bound():
    protos = header_prototypes()
    L = _lib.lib()
    for name, sig in ENTRIES.items():
        assert protos.get(name) == sig, (name, protos.get(name))
        assert hasattr(L, name), f"{name} not exported"
        assert _lib._SIGS.get(name) == sig, (name, _lib._SIGS.get(name))
        assert len(getattr(L, name).argtypes) == len(sig)
        assert name in _lib.EXPORTED
    assert protos.get("pm_sample_hash") == "uuuu" and "pm_sample_hash" in _lib.EXPORTED
    assert L.pm_sample_hash.argtypes == [ctypes.c_uint32] * 4 and L.pm_sample_hash.restype is ctypes.c_uint32
    assert protos["pm_mtp_from_logits"] == "ppilppps" and protos["pm_dropout_hash"] == "uuuu"
    src = open(HEADER).read()
    assert "sampled generation" in src
    assert re.search(r"uint32_t\s+pm_sample_hash\s*\(\s*uint32_t seed,\s*uint32_t row,\s*uint32_t head,\s*uint32_t token\s*\)", src)


def test_sampling_abi_version_is_unchanged():
    src = open(HEADER).read()
    assert int(re.search(r"#define PM_ABI_VERSION (\d+)", src).group(1)) == 9 == _lib.ABI_VERSION == _lib.lib().pm_abi_version()


@pytest.mark.parametrize("bad", [dict(c_logits=None), dict(tokens=None), dict(rows=0), dict(rows=-15), dict(rows=1 << 32),
                                 dict(rows=(1 << 32) + 15), dict(temperature=-1.0), dict(temperature=-1e-30),
                                 dict(temperature=float("nan")), dict(temperature=float("inf")), dict(top_k=-1),
                                 dict(top_k=-(1 << 31)), dict(top_p=0.0), dict(top_p=-0.5), dict(top_p=1.0000001),
                                 dict(top_p=2.0), dict(top_p=float("nan")), dict(top_p=float("inf"))],
                         ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()))
def test_sample_tokens_rejects_on_the_host(bad):
    assert _sample(**bad) == PM_E_INVALID
    assert _sample(**{**bad, "temperature": bad.get("temperature", 0.0)}) == PM_E_INVALID        # the greedy route too
    assert _sample(**{**dict(top_k=5, top_p=0.9), **bad}) == PM_E_INVALID                      # ... and the filtered one


@pytest.mark.parametrize("bad", [dict(tokens=None), dict(s=None), dict(bars=None), dict(ptr=None), dict(mtp=None), dict(G=0),
                                 dict(G=-1), dict(N=-1), dict(ptr=BARS), dict(G=1 << 29)],
                         ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()))
def test_mtp_from_tokens_rejects_what_mtp_from_logits_rejects(bad):
    assert _mtp(**bad) == PM_E_INVALID
    names = dict(tokens="c_logits", s="s_tensor", bars="bar_nodes", ptr="node_ptr")
    L = _lib.lib()
    args = dict(c_logits=LOGITS, s_tensor=S, G=2, N=7, bar_nodes=BARS, node_ptr=PTR, mtp=MTP)
    args.update({names.get(k, k): v for k, v in bad.items()})
    assert L.pm_mtp_from_logits(*args.values(), None) == PM_E_INVALID


def test_sample_hash_equals_the_numpy_replica():
    rng = np.random.default_rng(5)
    n = 10000
    seed, row, token = (rng.integers(0, 1 << 32, n, dtype=np.uint64) for _ in range(3))
    head = rng.integers(0, 2, n, dtype=np.uint64)
    token[: n // 2] %= np.uint64(131)                      # half of them real tokens, half any 32-bit word
    row[:4] = [0, 1, (1 << 32) - 1, (1 << 32) - 2]
    seed[:4] = [0, (1 << 32) - 1, (1 << 32) - 1, 0]
    want = sample_hash_np(seed, row, head, token)
    L = _lib.lib()
    got = np.array([L.pm_sample_hash(int(s), int(r), int(h), int(t)) for s, r, h, t in zip(seed, row, head, token)], np.uint64)
    assert np.array_equal(got, want)
    assert int(got.max()) < 1 << 23 and int(row.max()) == (1 << 32) - 1


def test_sample_stream_statistics():
    """The uniformity checks test_dropout_stream_statistics_and_numpy_replica applies to the dropout stream, on the 23-bit
    words of the sampling stream: the rate of words under p 2^23 is p, and the tokens of one row, the two heads of a row,
    neighbouring rows and two seeds fall under it independently (joint rate p^2), all within four standard deviations."""
    p = 0.1
    rows = np.arange(20000, dtype=np.uint64)[:, None]
    tok = np.arange(99, dtype=np.uint64)[None, :]
    thr = np.uint64(int(p * (1 << 23)))
    low = sample_hash_np(77, rows, 0, tok) < thr                                     # [rows, tokens]
    L = _lib.lib()
    for r in (0, 1, 4097, 19999):
        for t in (0, 1, 2, 63, 64, 98):
            assert (L.pm_sample_hash(77, r, 0, t) < int(thr)) == bool(low[r, t])
    one_row = sample_hash_np(77, 12345, 0, np.arange(1 << 16, dtype=np.uint64)) < thr      # the words of one row
    for x in (low, one_row):
        assert abs(x.mean() - p) < 4 * (p * (1 - p) / x.size) ** 0.5
    sig2 = lambda n: 4 * (p * p * (1 - p * p) / n) ** 0.5                             # 4 sigma of a joint rate
    assert abs((one_row[:-1] & one_row[1:]).mean() - p * p) < sig2(one_row.size - 1)
    assert abs((low[:, :-1] & low[:, 1:]).mean() - p * p) < sig2(low[:, 1:].size)     # same row, next token
    assert abs((low[:-1] & low[1:]).mean() - p * p) < sig2(low[1:].size)              # same token, next row
    for other in (sample_hash_np(77, rows, 1, tok) < thr, sample_hash_np(78, rows, 0, tok) < thr):   # other head, next seed
        assert abs((low & other).mean() - p * p) < sig2(low.size)
    u = (sample_hash_np(77, rows, 0, tok).astype(np.float64) + 0.5) / (1 << 23)
    assert 0 < u.min() and u.max() < 1 and abs(u.mean() - 0.5) < 4 * (1 / 12 / u.size) ** 0.5


BAD = [("temperature", v) for v in (-1.0, -1e-9, float("nan"), float("inf"), -float("inf"), True, False, "1.0", [1.0])] + \
      [("top_k", v) for v in (0, -1, 1.5, 5.0, True, "5")] + \
      [("top_p", v) for v in (0, 0.0, -0.1, 1.0000001, 2, float("nan"), float("inf"), True, "0.9")] + \
      [("seed", v) for v in (-1, 1 << 32, 1.0, True, "7")]


@pytest.mark.parametrize("name,value", BAD, ids=[f"{n}={v!r}" for n, v in BAD])
def test_generate_music_and_sample_tokens_reject_bad_sampling_arguments(name, value):
    """Before the model (None here) is touched, naming the argument."""
    from polyphemus_amd import ops
    from polyphemus_amd.generate import generate_music
    with pytest.raises(ValueError, match=name):
        generate_music(None, None, **{name: value})
    with pytest.raises(ValueError, match=name):
        generate_music(None, None, **{"temperature": 1.0, "top_k": 5, "top_p": 0.9, "seed": 1, name: value})
    with pytest.raises(ValueError, match=name):
        ops.sample_tokens(None, **{name: value})


def test_sampling_arguments_that_are_fine():
    from polyphemus_amd import ops
    for kw in (dict(), dict(temperature=0), dict(temperature=0.0), dict(temperature=1e-3), dict(temperature=np.float32(2)),
               dict(top_k=1), dict(top_k=np.int64(131)), dict(top_k=10 ** 6), dict(top_p=1), dict(top_p=1e-9),
               dict(top_p=np.float32(0.5)), dict(seed=0), dict(seed=(1 << 32) - 1), dict(seed=np.int64(5))):
        ops.check_sampling_args(**kw)
