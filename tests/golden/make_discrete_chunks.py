"""Records what the reference's get_discrete_chunks returns on a few small state paths:
tests/golden/discrete_chunks.json = [{"states": [per-trial lists], "include_edges": bool, "chunks": [per-state lists
of [chunk, beg, end]]}].  Data only -- inputs and expected outputs.  Run with the reference package on PYTHONPATH:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_discrete_chunks.py
"""
import json
import os

import numpy as np


def main():
    from behavenet.plotting.arhmm_utils import get_discrete_chunks
    rng = np.random.RandomState(5)
    cases = [
        [[0, 0, 0, 0]],                                            # a single run
        [[0, 1, 0, 1, 0, 1]],                                      # alternating
        [[0, 0, 2, 2, 2, 0]],                                      # state 1 never occurs
        [[1, 1, 0, 0, 1], [1, 0, 0, 0, 0], [0, 1, 1, 1, 1]],       # runs that touch each edge
        [[2], [0, 0, 1], [1]],                                     # one-frame trials
        [[3, 3, 1, 1, 1, 0, 2, 2, 3], [3, 0, 0, 0, 1, 2, 2]],
    ]
    for n_trials, length, K in ((4, 30, 3), (3, 57, 5)):
        # sticky random paths
        cases.append([np.repeat(rng.randint(0, K, size=length), rng.randint(1, 5, size=length))[:length].tolist()
                      for _ in range(n_trials)])
    out = []
    for states in cases:
        for include_edges in (True, False):
            got = get_discrete_chunks([np.asarray(s) for s in states], include_edges=include_edges)
            out.append({'states': states, 'include_edges': include_edges,
                        'chunks': [np.asarray(c).reshape(-1, 3).astype(int).tolist() for c in got]})
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'discrete_chunks.json')
    with open(path, 'w') as f:
        json.dump(out, f, sort_keys=True)
    print('%d cases -> %s' % (len(out), path))


if __name__ == '__main__':
    main()
