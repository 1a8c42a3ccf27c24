"""The host side of the states of a grid of ARHMMs: the workspace restatement, the wrappers' argument checks, the
selection table on hand-made rows and runs, and what check_export_arhmm_grid refuses.  No GPU."""

import numpy as np
import pytest
import torch

from behavenet_amd import _hip
from behavenet_amd.fitting.eval import arhmm_grid_selection, check_export_arhmm_grid


@pytest.mark.parametrize('n,S,Ks', [(0, 1, [3]), (583, 9, [1, 4] * 20), (4000, 7, [17, 32, 17]), (10 ** 6, 1000, [12] * 31),
                                    (1, 1, [1]), (4097, 3, [32] * 16)])
def test_the_restated_workspace_is_the_library_s(n, S, Ks):
    lib = _hip.load()
    M, KT, XT = len(Ks), sum(Ks), sum(k * k for k in Ks)
    assert lib.bn_hmm_grid_viterbi_ws_bytes(n, S, M, KT, XT) == _hip.hmm_grid_viterbi_ws_bytes(n, S, Ks)
    assert _hip.hmm_grid_viterbi_ws_bytes(n, S, Ks) >= (S + 1) * 4 + n * KT


def test_the_query_refuses_what_the_call_refuses():
    lib = _hip.load()
    # (n, S, M, KT, XT): no models, more models than states, 513 states, XT outside [KT, 32 KT]
    for args in ((10, 1, 0, 40, 100), (10, 1, 41, 40, 100), (10, 1, 20, 513, 600), (10, 1, 20, 40, 39),
                 (10, 1, 20, 40, 1281), (-1, 1, 20, 40, 100)):
        assert lib.bn_hmm_grid_viterbi_ws_bytes(*args) == 0
    vit = lambda M, KT, XT, counts: lib.bn_hmm_grid_viterbi(None, None, 1, M, KT, XT, 10, None, None, None, *counts,
                                                            None, None, None, None, 0, None)
    assert vit(20, 513, 600, (20, 0, 0, 0)) == -2
    assert vit(20, 40, 100, (19, 0, 0, 0)) == -2             # the classes do not add up to the models
    assert vit(20, 40, 100, (21, -1, 0, 0)) == -2
    assert vit(20, 40, 100, (20, 0, 0, 0)) == -1             # NULL operands with shapes that are served


def test_hmm_grid_viterbi_checks_its_arguments():
    ll = torch.zeros((10, 40), dtype=torch.float64)
    Ks = [8] * 5
    with pytest.raises(ValueError, match='hmm_grid_viterbi.*no CPU fallback'):
        _hip.hmm_grid_viterbi(ll, [0, 10], Ks, np.zeros(5 * 64), np.zeros(40))
    with pytest.raises(ValueError, match='float64'):
        _hip.hmm_grid_viterbi(ll.float(), [0, 10], Ks, np.zeros(5 * 64), np.zeros(40))
    with pytest.raises(ValueError, match=r'\(n, 41\)'):
        _hip.hmm_grid_viterbi(ll, [0, 10], Ks + [1], np.zeros(5 * 64 + 1), np.zeros(41))
    with pytest.raises(ValueError, match='33 states'):
        _hip.hmm_grid_viterbi(ll, [0, 10], [33, 7], np.zeros(33 * 33 + 49), np.zeros(40))
    with pytest.raises(ValueError, match='513 states'):
        _hip.hmm_grid_viterbi(torch.zeros((4, 513), dtype=torch.float64), [0, 4], [27] * 19, np.zeros(19 * 27 * 27),
                              np.zeros(513))
    with pytest.raises(ValueError, match='0 models'):
        _hip.hmm_grid_viterbi(ll, [0, 10], [], np.zeros(0), np.zeros(0))


def test_state_runs_grid_checks_its_arguments():
    states = torch.zeros((3, 10), dtype=torch.int32)
    with pytest.raises(ValueError, match='state_runs_grid.*no CPU fallback'):
        _hip.state_runs_grid(states, [0, 10], [2, 3, 4])
    with pytest.raises(ValueError, match=r'int32 \(M, n\)'):
        _hip.state_runs_grid(states.long(), [0, 10], [2, 3, 4])
    with pytest.raises(ValueError, match=r'int32 \(M, n\)'):
        _hip.state_runs_grid(states[0], [0, 10], [2])
    with pytest.raises(ValueError, match=r'int32 \(M, n\)'):
        _hip.state_runs_grid(np.zeros((3, 10), dtype=np.int32), [0, 10], [2, 3, 4])


# ------------------------------------------------------------------------------------------------------------
# arhmm_grid_selection
# ------------------------------------------------------------------------------------------------------------
def _rows(n_epochs, tr, val, tests):
    rows = []
    for epoch in range(n_epochs):
        for d in (-1, 0, 1):
            rows.append({'epoch': epoch, 'dataset': d, 'tr_loss': tr + d - epoch, 'val_loss': val + d - epoch,
                         'trial': -1})
    for (d, trial), loss in tests:
        rows.append({'epoch': n_epochs - 1, 'dataset': d, 'test_loss': loss, 'trial': trial})
    return rows


def _runs(rows):
    return np.asarray(rows, dtype=np.int32).reshape(-1, 4)


def test_selection_on_hand_made_rows_and_runs():
    grid = [{'n_states': 4, 'kappa': 0}, {'n_states': 3, 'n_lags': 2}, {'n_states': 2}, {'n_states': 1}]
    tests = [((0, 5), 2.0), ((1, 2), 4.0), ((1, 7), float('nan'))]
    fits = [(None, _rows(3, 10.0, 20.0, tests)), (None, _rows(1, 1.0, 2.0, [])), (None, _rows(2, 5.0, 6.0, tests)),
            (None, _rows(2, 5.0, 6.0, tests[:1]))]
    stats = [
        # ties in usage (40, 40), a state with zero frames; runs over two trials, edges included
        (_runs([[0, 0, 40, 0], [0, 40, 60, 3], [1, 0, 40, 1]]), np.asarray([40, 40, 0, 20]), np.zeros((4, 4))),
        None,                                               # a model without stats
        (_runs([[0, 0, 7, 1]]), np.asarray([0, 7]), np.zeros((2, 2))),                  # a single run
        (np.zeros((0, 4), dtype=np.int32), np.asarray([0]), np.zeros((1, 1))),          # no frames at all
    ]
    frames = {(0, 5): 10, (1, 2): 30, (1, 7): 0}
    table = arhmm_grid_selection(grid, fits, stats, test_frames=frames)
    assert len(table) == 4
    a, b, c, d = table
    assert (a['n_states'], a['kappa']) == (4, 0) and 'n_lags' not in a      # the configuration's own keys
    assert (b['n_states'], b['n_lags']) == (3, 2)
    # the last epoch's POOLED losses (dataset == -1), not the last session's
    assert (a['epochs'], a['tr_loss'], a['val_loss']) == (2, 10.0 - 1 - 2, 20.0 - 1 - 2)
    assert (b['epochs'], b['tr_loss'], b['val_loss']) == (0, 0.0, 1.0)
    assert a['test_loss'] == (10 * 2.0 + 30 * 4.0) / 40 and c['test_loss'] == a['test_loss']
    assert np.isnan(b['test_loss']) and d['test_loss'] == 2.0
    assert np.array_equal(a['usage'], [0.4, 0.4, 0.0, 0.2]) and a['usage'].dtype == np.float64
    assert (a['n_states_used'], a['n_states_99'], a['n_runs']) == (3, 3, 3)
    assert (a['median_duration'], a['mean_duration']) == (40.0, 100.0 / 3)
    for key in ('usage', 'n_states_used', 'n_states_99', 'n_runs', 'median_duration', 'mean_duration'):
        assert b[key] is None
    assert np.array_equal(c['usage'], [0.0, 1.0])
    assert (c['n_states_used'], c['n_states_99'], c['n_runs'], c['median_duration'], c['mean_duration']) == \
        (1, 1, 1, 7.0, 7.0)
    assert np.array_equal(d['usage'], [0.0]) and (d['n_states_used'], d['n_states_99'], d['n_runs']) == (0, 0, 0)
    assert np.isnan(d['median_duration']) and np.isnan(d['mean_duration'])
    # without the trials' frames every test trial weighs the same; without stats every run field is None
    plain = arhmm_grid_selection(grid, fits, None)
    assert plain[0]['test_loss'] == 3.0 and all(r['n_runs'] is None for r in plain)
    with pytest.raises(ValueError, match='4 configurations, 3 fits'):
        arhmm_grid_selection(grid, fits[:3], stats)


def test_the_99_percent_rule_is_exact_at_its_edge():
    fit = (None, _rows(1, 1.0, 1.0, []))
    for frames, want in (([99, 1], 1), ([98, 2], 2), ([980, 10, 10], 2), ([50, 49, 1], 2), ([25, 25, 25, 25], 4),
                         ([1, 98, 1], 2)):
        st = (np.zeros((0, 4), dtype=np.int32), np.asarray(frames), None)
        assert arhmm_grid_selection([{'n_states': len(frames)}], [fit], [st])[0]['n_states_99'] == want, frames


# ------------------------------------------------------------------------------------------------------------
# check_export_arhmm_grid
# ------------------------------------------------------------------------------------------------------------
def test_check_export_arhmm_grid_refusals():
    who = "fit: hparams['export_arhmm_grid']"
    ok = {'n_states': 2}
    check_export_arhmm_grid(who, {'grid': [ok, {'n_states': 32, 'n_lags': 8, 'transitions': 'sticky', 'kappa': 10}],
                                  'n_iters': 2, 'dtype': 'test', 'tol': 0, 'sess_idx': None,
                                  'data_key': 'ae_latents'})
    with pytest.raises(ValueError, match='export_arhmm_grid.*expected a dict with grid'):
        check_export_arhmm_grid(who, {'n_iters': 2})                               # a dict without grid
    with pytest.raises(ValueError, match='expected a dict with grid'):
        check_export_arhmm_grid(who, [ok])
    with pytest.raises(ValueError, match='expected a dict with grid'):
        check_export_arhmm_grid(who, {'grid': [ok], 'n_states': 2})                # a key the export does not take
    with pytest.raises(ValueError, match='non-empty list'):
        check_export_arhmm_grid(who, {'grid': []})
    with pytest.raises(ValueError, match='non-empty list'):
        check_export_arhmm_grid(who, {'grid': ok})
    with pytest.raises(ValueError, match='a configuration is a dict'):
        check_export_arhmm_grid(who, {'grid': [{'n_lags': 1}]})
    with pytest.raises(NotImplementedError, match="noise_type 'studentst'"):
        check_export_arhmm_grid(who, {'grid': [ok, {'n_states': 2, 'noise_type': 'studentst'}]})
    with pytest.raises(NotImplementedError, match='recurrent'):
        check_export_arhmm_grid(who, {'grid': [ok, {'n_states': 2, 'transitions': 'recurrent'}]})
    with pytest.raises(ValueError, match='33 states'):
        check_export_arhmm_grid(who, {'grid': [ok, {'n_states': 33}]})
    with pytest.raises(ValueError, match='9 lags'):
        check_export_arhmm_grid(who, {'grid': [{'n_states': 2, 'n_lags': 9}]})
    with pytest.raises(ValueError, match='dtype'):
        check_export_arhmm_grid(who, {'grid': [ok], 'dtype': 'all'})
    with pytest.raises(ValueError, match='dtype'):
        check_export_arhmm_grid(who, {'grid': [ok], 'dtype': ['val', 'test']})
    with pytest.raises(ValueError, match='data_key'):
        check_export_arhmm_grid(who, {'grid': [ok], 'data_key': 'frames'})
