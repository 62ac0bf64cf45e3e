"""C-ABI checks of the exponential moving average of the parameters that need no GPU: its two entries are declared in
include/polyphemus_hip.h, exported by the library and bound in the ctypes table with the header's argument list, the ABI
version is unchanged, and every argument check answers PM_E_INVALID on the host, before any launch (so host integers can
stand in for device addresses)."""
import re

import pytest

from polyphemus_amd import _lib
from test_abi import HEADER, header_prototypes

ENTRIES = {"pm_adam_step_ema": "ppppplffffiffpps", "pm_buffer_swap": "ppls"}
PM_E_INVALID = -1
# fake device addresses, 16-byte aligned and 1 MiB apart: n = 1024 floats (4 KiB) from one never reach the next
P, G, M, V, E, CLIP, STATUS = (0x10000000 + k * 0x100000 for k in range(7))
N = 1024
HYPER = (1e-3, 0.9, 0.98, 1e-9)            # lr, beta1, beta2, eps


def _ema(params=P, grads=G, exp_avg=M, exp_avg_sq=V, ema=E, n=N, step=1, grad_scale=1.0, w=0.1, clip=None, status=None):
    return _lib.lib().pm_adam_step_ema(params, grads, exp_avg, exp_avg_sq, ema, n, *HYPER, step, grad_scale, w, clip, status,
                                       None)


def test_ema_entries_declared_exported_and_bound():
    protos = header_prototypes()
    L = _lib.lib()
    for name, sig in ENTRIES.items():
        assert protos.get(name) == sig, (name, protos.get(name))
        assert hasattr(L, name), f"{name} not exported"
        assert _lib._SIGS.get(name) == sig, (name, _lib._SIGS.get(name))
        assert len(getattr(L, name).argtypes) == len(sig)
        assert name in _lib.EXPORTED
    # the entries it is the superset of keep their argument lists
    assert protos["pm_adam_step"] == "pppplffffifs" and protos["pm_adam_step_guarded"] == "pppplffffps"
    assert protos["pm_adam_step_clipped"] == "pppplffffipps"
    assert "exponential moving average of the parameters" in open(HEADER).read()


def test_ema_abi_version_is_unchanged():
    src = open(HEADER).read()
    assert int(re.search(r"#define PM_ABI_VERSION (\d+)", src).group(1)) == 9 == _lib.ABI_VERSION == _lib.lib().pm_abi_version()


@pytest.mark.parametrize("null", ["params", "grads", "exp_avg", "exp_avg_sq", "ema"])
def test_adam_step_ema_rejects_a_null_buffer(null):
    assert _ema(**{null: None}) == PM_E_INVALID


@pytest.mark.parametrize("w", [0.0, -0.5, 1.5, float("nan"), -0.0, float("inf")])
def test_adam_step_ema_rejects_a_weight_outside_0_1(w):
    assert _ema(w=w) == PM_E_INVALID
    assert _ema(w=w, clip=CLIP, status=STATUS) == PM_E_INVALID


@pytest.mark.parametrize("other", ["params", "grads", "exp_avg", "exp_avg_sq"])
def test_adam_step_ema_rejects_an_average_that_aliases_another_buffer(other):
    at = dict(params=P, grads=G, exp_avg=M, exp_avg_sq=V)[other]
    assert _ema(ema=at) == PM_E_INVALID                                 # the same buffer
    assert _ema(ema=at + 4 * (N - 1)) == PM_E_INVALID                   # its last element is the average's first
    assert _ema(ema=at - 4 * (N - 1)) == PM_E_INVALID                   # the average's last element is its first


def test_adam_step_ema_rejects_bad_sizes_steps_and_clip_alignment():
    assert _ema(n=0) == PM_E_INVALID and _ema(n=-4) == PM_E_INVALID
    assert _ema(step=0) == PM_E_INVALID and _ema(step=-1) == PM_E_INVALID           # status == NULL: the host's t, >= 1
    assert _ema(step=0, clip=CLIP) == PM_E_INVALID
    assert _ema(clip=CLIP + 4) == PM_E_INVALID and _ema(clip=CLIP + 4, status=STATUS, step=0) == PM_E_INVALID


def test_buffer_swap_rejects_null_empty_and_overlapping_ranges():
    swap = _lib.lib().pm_buffer_swap
    assert swap(None, G, N, None) == PM_E_INVALID and swap(P, None, N, None) == PM_E_INVALID
    assert swap(P, G, 0, None) == PM_E_INVALID and swap(P, G, -1, None) == PM_E_INVALID
    assert swap(P, P, N, None) == PM_E_INVALID
    for d in (4, 16, 4 * (N - 1)):                                      # one element .. all but one shared, both orders
        assert swap(P, P + d, N, None) == PM_E_INVALID, d
        assert swap(P + d, P, N, None) == PM_E_INVALID, d


@pytest.mark.parametrize("bad", [True, False, -0.1, 1.0, 1.5, "0.9", 1 - 1e-12, float("nan")])
def test_trainer_rejects_bad_ema_decay(bad):
    """Before the trainer touches the model.  1 - 1e-12 is 1 as a float32: an average that could never move."""
    from polyphemus_amd.trainer import HipTrainer
    with pytest.raises(ValueError, match="ema_decay"):
        HipTrainer.__init__(object.__new__(HipTrainer), None, ema_decay=bad)


def test_ema_weight_is_float32_of_the_double_difference():
    import numpy as np
    from polyphemus_amd import ops
    for decay in (0, 0.0, 0.5, 0.9, 0.999, 0.9999, 1 - 2.0 ** -24):
        assert ops.ema_weight(decay) == float(np.float32(1.0 - float(decay)))
    assert ops.ema_weight(0) == 1.0
