"""The scores of pm_score_tokens and pm_score_structure ("Scores", include/polyphemus_hip.h) restated in numpy float64, and
the inputs the tests of both share.  The restatement derives node -> (bar, track) from the structure in cell order and takes
hits with np.argmax (the first index on ties)."""
import numpy as np

N_PITCH, N_DUR, N_TOK, SLOTS = 131, 99, 230, 15
PITCH_SOS, PITCH_EOS, PITCH_PAD, DUR_SOS, DUR_EOS, DUR_PAD = 128, 129, 130, 96, 97, 98
V_PITCH_HIT, V_DUR_HIT, V_PITCH_SET, V_DUR_SET = 1, 2, 4, 8


def _log_softmax64(x):
    x = x.astype(np.float64)
    m = x.max(axis=-1, keepdims=True)
    return (x - m) - np.log(np.exp(x - m).sum(axis=-1, keepdims=True))


def node_cells(s_tensor):
    """(bar, track) of every node of a structure [..., 4, 32]: the active cells in cell order."""
    s = np.asarray(s_tensor).reshape(-1, 128) != 0
    bar, cell = np.nonzero(s)
    return bar, cell // 32


def targets_of(tokens):
    """The 15 target pairs of every node: tokens [N,15,2], or [N,16,2] whose slot 0 (the SOS) is dropped."""
    tokens = np.asarray(tokens)
    assert tokens.ndim == 3 and tokens.shape[1] in (SLOTS, SLOTS + 1) and tokens.shape[2] == 2
    return tokens[:, tokens.shape[1] - SLOTS:]


def score_rows_ref(c_logits, tokens):
    """(row_logp float64 [N,15,2], verdict uint8 [N,15]) of pm_score_tokens."""
    x, t = np.asarray(c_logits), targets_of(tokens).astype(np.int64)
    N = x.shape[0]
    row_logp, verdict = np.zeros((N, SLOTS, 2)), np.zeros((N, SLOTS), np.uint8)
    for h, (lo, hi, pad, hit, present) in enumerate(((0, N_PITCH, PITCH_PAD, V_PITCH_HIT, V_PITCH_SET),
                                                     (N_PITCH, N_TOK, DUR_PAD, V_DUR_HIT, V_DUR_SET))):
        head, th = x[:, :, lo:hi], t[:, :, h]
        on = (th >= 0) & (th < pad)
        lp = np.take_along_axis(_log_softmax64(head), np.where(on, th, 0)[..., None], axis=-1)[..., 0]
        row_logp[:, :, h] = np.where(on, lp, 0.0)
        verdict |= (on * present + (on & (np.argmax(head, axis=-1) == th)) * hit).astype(np.uint8)
    return row_logp, verdict


def score_tokens_ref(c_logits, tokens, s_tensor, N=None):
    """(logp float64 [G,4,2], counts int32 [G,4,6], row_logp float64 [N,15,2], verdict uint8 [N,15]); nodes at N and beyond
    are ignored."""
    row_logp, verdict = score_rows_ref(c_logits, tokens)
    N = row_logp.shape[0] if N is None else N
    G = np.asarray(s_tensor).reshape(-1, 128).shape[0]
    logp, counts = np.zeros((G, 4, 2)), np.zeros((G, 4, 6), np.int32)
    for n, (g, k) in enumerate(zip(*node_cells(s_tensor))):
        if n >= N:
            break
        v = verdict[n].astype(np.int64)
        logp[g, k] += row_logp[n].sum(axis=0)
        both = V_PITCH_HIT | V_DUR_HIT
        counts[g, k] += np.array([1, ((v & V_PITCH_SET) != 0).sum(), ((v & V_DUR_SET) != 0).sum(), ((v & V_PITCH_HIT) != 0).sum(),
                                  ((v & V_DUR_HIT) != 0).sum(), ((v & both) == both).sum()], np.int32)
    return logp, counts, row_logp, verdict


def structure_terms_ref(s_logits, s_tensor):
    """The Bernoulli terms max(x, 0) - x y + log1p(exp(-|x|)) of every cell in float64, [G,4,32]."""
    x = np.asarray(s_logits).astype(np.float64).reshape(-1, 4, 32)
    y = (np.asarray(s_tensor).reshape(-1, 4, 32) != 0).astype(np.float64)
    return np.maximum(x, 0.0) - x * y + np.log1p(np.exp(-np.abs(x)))


def score_structure_ref(s_logits, s_tensor):
    """(logp float64 [G,4], counts int32 [G,4,4] = targets on, predictions on, true positives, cells that agree); the
    prediction is sigmoid(x) >= 0.5 evaluated in float32 as the metrics kernel does, which is x >= 0."""
    x32 = np.asarray(s_logits).astype(np.float32).reshape(-1, 4, 32)
    y = np.asarray(s_tensor).reshape(-1, 4, 32) != 0
    with np.errstate(over="ignore"):
        pred = (np.float32(1) / (np.float32(1) + np.exp(-x32))) >= np.float32(0.5)
    counts = np.stack([y.sum(-1), pred.sum(-1), (y & pred).sum(-1), (y == pred).sum(-1)], axis=-1).astype(np.int32)
    return -structure_terms_ref(s_logits, s_tensor).sum(-1), counts


# ---- the inputs of the tests -----------------------------------------------------------------------------------------

def structures():
    """name -> bool [B,n_bars,4,32]: one bar with one node; three bars (odd: the last half-wave has no bar) = a full bar of
    128 nodes, a bar with an empty track, a bar whose only node is cell [0,0]; two pieces of two bars at density 0.3."""
    rng = np.random.default_rng(20)
    one = np.zeros((1, 1, 4, 32), bool)
    one[0, 0, 2, 17] = True
    three = np.zeros((1, 3, 4, 32), bool)
    three[0, 0] = True
    three[0, 1] = rng.random((4, 32)) < 0.4
    three[0, 1, 2] = False
    three[0, 1, 3, 31] = True
    three[0, 2, 0, 0] = True
    dense = rng.random((2, 2, 4, 32)) < 0.3
    return {"one_node": one, "three_bars": three, "two_pieces": dense}


PLANTED = ("both PAD", "pitch PAD only", "duration PAD only", "tie, target first", "tie, target second", "pitch head + 80",
           "duration head - 80", "a column at -inf")


def token_case(s_tensor, tok_slots, seed):
    """(c_logits float32 [N,15,230] ~ N(0, 3^2), tokens int32 [N,tok_slots,2]) for a structure: every node holds k notes, an
    EOS and PAD behind it; the rows j < len(PLANTED) of node 0 (and of node 5 and the last node, where there are such) carry
    the planted cases in that order."""
    rng = np.random.default_rng(seed)
    N = int(np.count_nonzero(s_tensor))
    x = (3.0 * rng.standard_normal((N, SLOTS, N_TOK))).astype(np.float32)
    t = np.empty((N, SLOTS, 2), np.int32)
    t[:, :, 0], t[:, :, 1] = PITCH_PAD, DUR_PAD
    for n in range(N):
        k = int(rng.integers(0, SLOTS))
        t[n, :k, 0], t[n, :k, 1] = rng.integers(0, 128, k), rng.integers(0, 96, k)
        t[n, k] = (PITCH_EOS, DUR_EOS)
    for n in sorted({0, min(5, N - 1), N - 1}):
        t[n, :8, 0], t[n, :8, 1] = rng.integers(0, 128, 8), rng.integers(0, 96, 8)
        t[n, 0] = (PITCH_PAD, DUR_PAD)
        t[n, 1, 0] = PITCH_PAD
        t[n, 2, 1] = DUR_PAD
        for j, first in ((3, True), (4, False)):                                 # exact ties at the max, in both heads
            for h, lo, size in ((0, 0, N_PITCH), (1, N_PITCH, N_DUR)):
                a, b = sorted(rng.choice(size, 2, replace=False))
                top = np.float32(x[n, j, lo:lo + size].max() + 1.0)
                x[n, j, lo + a] = x[n, j, lo + b] = top
                t[n, j, h] = a if first else b
        x[n, 5, :N_PITCH] += np.float32(80.0)
        x[n, 6, N_PITCH:] -= np.float32(80.0)
        for h, lo, size in ((0, 0, N_PITCH), (1, N_PITCH, N_DUR)):               # a column that is not the target
            x[n, 7, lo + (t[n, 7, h] + 1 + int(rng.integers(0, size - 1))) % size] = -np.inf
    if tok_slots == SLOTS + 1:
        sos = np.empty((N, 1, 2), np.int32)
        sos[:, 0] = (PITCH_SOS, DUR_SOS)
        t = np.concatenate([sos, t], axis=1)
    return x, np.ascontiguousarray(t)


def structure_case(G, seed):
    """(s_logits float32 [1,G,4,32] ~ N(0, 2^2) with +-100 and exact zeros planted on cells that are on and cells that are
    off, s_tensor bool [1,G,4,32])."""
    rng = np.random.default_rng(seed)
    x = (2.0 * rng.standard_normal((1, G, 4, 32))).astype(np.float32)
    y = rng.random((1, G, 4, 32)) < 0.4
    for k, (v, on) in enumerate(((100.0, True), (100.0, False), (-100.0, True), (-100.0, False), (0.0, True), (0.0, False),
                                 (-0.0, True))):
        x[0, G - 1, k % 4, 3 + 2 * k] = v
        y[0, G - 1, k % 4, 3 + 2 * k] = on
    return x, y
