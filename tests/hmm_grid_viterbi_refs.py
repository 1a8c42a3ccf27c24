"""Float64 restatements for the states of a grid of ARHMMs (bn_hmm_grid_viterbi, state_runs_grid, ARHMMGroup's
decoding half): max-sum forwards and backwards -- two independent values of the same maximum -- the score of a given
path, every path of a tiny trial, and the grids the GPU tests share.  numpy only; nothing here touches the device."""

import itertools

import numpy as np

# the classes of the packing and the state counts at both ends of each
CLASSES = (4, 8, 16, 32)
CLASS_ENDS = {4: (1, 4), 8: (5, 8), 16: (9, 16), 32: (17, 32)}
# empty trials, single rows and both sides of the 64-row walk-back chunk; two rows in front belong to no trial
LENGTHS = [0, 1, 2, 63, 64, 65, 129, 257, 0]
FRONT, BACK = 2, 2
KINDS = ('random', 'absorbing', 'uniform')


def trials_of(offsets):
    e = np.maximum.accumulate(np.asarray(offsets, dtype=np.int64))
    return [(int(e[s]), int(e[s + 1])) for s in range(len(e) - 1)]


def class_ks(KP):
    """Two full waves of the class and a partly filled third, the state counts alternating between the class's ends."""
    lo, hi = CLASS_ENDS[KP]
    slots = 64 // KP
    count = 2 * slots + max(1, slots // 2)
    return [lo if m % 2 == 0 else hi for m in range(count)]


def mixed_ks():
    """Every class three times, interleaved: the order the launcher has to sort."""
    return [1, 4, 5, 8, 9, 16, 17, 32] * 3


def random_hmm(rng, K, kind='random'):
    if kind == 'uniform':
        Ps = np.full((K, K), 1.0 / K)
    elif kind == 'absorbing':
        Ps = np.full((K, K), 1e-9) + np.eye(K)
    else:
        Ps = rng.rand(K, K) + 0.1
    Ps /= Ps.sum(axis=1, keepdims=True)
    pi0 = rng.rand(K) + 0.1
    pi0 /= pi0.sum()
    return np.log(Ps), np.log(pi0)


def hmm_grid(seed, Ks, lengths=LENGTHS):
    """ll in [-1e4, -1e4 + 50] and the transition kinds in turn: (ll (n, KT), offsets, [(log_Ps, log_pi0)])."""
    rng = np.random.RandomState(seed)
    offsets = np.cumsum([FRONT] + list(lengths)).astype(np.int64)
    ll = -1e4 + 50.0 * rng.rand(int(offsets[-1]) + BACK, int(np.sum(Ks)))
    hmms = [random_hmm(rng, K, KINDS[m % 3]) for m, K in enumerate(Ks)]
    return ll, offsets, hmms


def packed(hmms):
    """(log_Ps (XT,), log_pi0 (KT,)) as the grid wrappers take them."""
    return np.concatenate([h[0].reshape(-1) for h in hmms]), np.concatenate([h[1] for h in hmms])


def columns(Ks):
    koff = np.concatenate(([0], np.cumsum(Ks))).astype(np.int64)
    return [(int(koff[m]), int(koff[m + 1])) for m in range(len(Ks))]


def path_score(ll, log_Ps, log_pi0, path):
    """log pi0 + sum of transitions and emissions along ``path``, added in row order."""
    ll = np.asarray(ll, dtype=np.float64)
    if len(path) == 0:
        return 0.0
    s = log_pi0[path[0]] + ll[0, path[0]]
    for t in range(1, len(path)):
        s += log_Ps[path[t - 1], path[t]] + ll[t, path[t]]
    return float(s)


def viterbi(ll, log_Ps, log_pi0):
    """Max-sum from the first row to the last, ties to the lowest state: (path, maximum)."""
    ll = np.asarray(ll, dtype=np.float64)
    T, K = ll.shape
    if T == 0:
        return np.zeros((0,), dtype=np.int32), 0.0
    delta = log_pi0 + ll[0]
    back = np.zeros((T, K), dtype=np.int64)
    for t in range(1, T):
        cand = delta[:, None] + log_Ps
        back[t] = np.argmax(cand, axis=0)
        delta = cand[back[t], np.arange(K)] + ll[t]
    path = np.zeros(T, dtype=np.int32)
    path[T - 1] = int(np.argmax(delta))
    for t in range(T - 1, 0, -1):
        path[t - 1] = back[t, path[t]]
    return path, float(np.max(delta))


def viterbi_backward(ll, log_Ps, log_pi0):
    """The same maximum from the last row to the first (another order of the same sums): the value alone."""
    ll = np.asarray(ll, dtype=np.float64)
    T, K = ll.shape
    if T == 0:
        return 0.0
    beta = np.zeros(K)
    for t in range(T - 1, 0, -1):
        beta = np.max(log_Ps + (ll[t] + beta)[None, :], axis=1)
    return float(np.max(log_pi0 + ll[0] + beta))


def brute_force(ll, log_Ps, log_pi0):
    """Every path of a tiny trial: (the best path, the first in lexicographic order among equals, its score)."""
    ll = np.asarray(ll, dtype=np.float64)
    T, K = ll.shape
    paths = list(itertools.product(range(K), repeat=T))
    scores = np.asarray([path_score(ll, log_Ps, log_pi0, p) for p in paths])
    best = int(np.argmax(scores))
    return np.asarray(paths[best], dtype=np.int32), float(scores[best])
