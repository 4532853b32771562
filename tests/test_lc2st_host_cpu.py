"""Host side of L-C2ST (sbi_amd/diagnostics/lc2st.py) without a GPU: the state machine and its messages, validation,
NaN removal, z-scoring, how members are built (null permutations, folds, validation split), the p-value from injected
scores, every refusal, the oracle's early-stopping bookkeeping, and the C header against the ctypes table."""
import ctypes
import os
import re
import warnings

import numpy as np
import pytest
import torch

from sbi_amd import _build, _lib
from sbi_amd.diagnostics import LC2ST, LC2ST_NF, LC2STScores, LC2STState, permute_data
from sbi_amd.diagnostics import lc2st as L
from tests import lc2st_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _data(n=50, d=2, dx=3, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, d, generator=g), torch.randn(n, dx, generator=g), torch.randn(n, d, generator=g)


def test_state_machine_and_messages():
    th, x, post = _data()
    lc = LC2ST(th, x, post, num_trials_null=3)
    assert lc.state == LC2STState.INITIALIZED
    with pytest.raises(RuntimeError, match=r"Call train_on_observed_data\(\) and train_under_null_hypothesis\(\) first"):
        lc.p_value(th, x[0])
    with pytest.raises(RuntimeError, match="have not been trained on observed data"):
        lc.get_statistic_on_observed_data(th, x[0])
    with pytest.raises(RuntimeError, match="have not been trained under the null hypothesis"):
        lc.get_statistics_under_null_hypothesis(th, x[0])
    lc._state = LC2STState.OBSERVED_TRAINED
    with pytest.raises(RuntimeError, match=r"Call train_under_null_hypothesis\(\) first"):
        lc.p_value(th, x[0])
    lc._state = LC2STState.NULL_TRAINED
    with pytest.raises(RuntimeError, match=r"Call train_on_observed_data\(\) first"):
        lc.reject_test(th, x[0])
    with pytest.raises(RuntimeError, match="Expected 3 null classifiers, got 0"):
        lc.get_statistics_under_null_hypothesis(th, x[0])
    lc.trained_clfs_null = {0: []}
    with pytest.raises(ValueError, match="already trained"):
        lc.train_under_null_hypothesis()
    lc2 = LC2ST(th, x, post, permutation=False)
    with pytest.raises(ValueError, match="A null distribution must be provided when permutation=False"):
        lc2.train_under_null_hypothesis()


@pytest.mark.skipif(torch.cuda.is_available(), reason="a ROCm device is visible")
def test_without_a_device_training_raises():
    th, x, post = _data()
    with pytest.raises(RuntimeError, match="only on a ROCm device"):
        LC2ST(th, x, post).train_on_observed_data()
    with pytest.raises(RuntimeError, match="only on a ROCm device"):
        L.lc2st_eval(L.LC2STHyper(2, 3, 20), torch.zeros(1, 20 * 5 + 400 + 61), th, x[0])


def test_validation_and_deprecations():
    th, x, post = _data()
    for kw, err, msg in [
        (dict(xs=x, posterior_samples=post), ValueError, "prior_samples is required"),
        (dict(prior_samples=th, posterior_samples=post), ValueError, "xs is required"),
        (dict(prior_samples=th, xs=x), ValueError, "posterior_samples is required"),
        (dict(prior_samples=th.numpy(), xs=x, posterior_samples=post), TypeError, "prior_samples must be a torch.Tensor"),
        (dict(prior_samples=th[:0], xs=x, posterior_samples=post), ValueError, "prior_samples cannot be empty"),
        (dict(prior_samples=th[:10], xs=x, posterior_samples=post), ValueError, "Sample size mismatch"),
        (dict(prior_samples=th, xs=x, posterior_samples=post[:, :1]), ValueError, "Dimension mismatch"),
        (dict(prior_samples=th, xs=x, posterior_samples=post, num_folds=0), ValueError, "num_folds must be >= 1"),
        (dict(prior_samples=th, xs=x, posterior_samples=post, num_folds=51), ValueError, "cannot exceed sample size"),
        (dict(prior_samples=th, xs=x, posterior_samples=post, seed=1.5), TypeError, "seed must be an integer"),
        (dict(prior_samples=th, xs=x, posterior_samples=post, thetas=th), ValueError, "Cannot specify both"),
    ]:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            with pytest.raises(err, match=msg):
                LC2ST(**kw)
    with pytest.warns(FutureWarning, match="'thetas' is deprecated"):
        lc = LC2ST(xs=x, posterior_samples=post, thetas=th)
    assert torch.equal(lc.theta_q, th)
    with pytest.raises(ValueError, match="flow_inverse_transform is required"):
        LC2ST_NF(th, x, post)
    with pytest.raises(ValueError, match="flow_base_dist is required"):
        LC2ST_NF(th, x, post, flow_inverse_transform=lambda a, b: a)


def test_nan_and_inf_rows_are_removed_everywhere():
    th, x, post = _data()
    x = x.clone()
    x[3, 0], x[7, 1], x[9, 2] = float("nan"), float("inf"), float("nan")
    with pytest.warns(UserWarning, match=r"Found 2 NaNs and 1 Infs in xs.*Only 47 / 50 samples remain"):
        lc = LC2ST(th, x, post)
    keep = [i for i in range(50) if i not in (3, 7, 9)]
    assert torch.equal(lc.theta_q, th[keep]) and torch.equal(lc.theta_p, post[keep]) and torch.equal(lc.x_p, x[keep])


def test_z_score_with_a_constant_column():
    th, x, post = _data()
    x = x.clone()
    x[:, 1] = 4.0
    lc = LC2ST(th, x, post, z_score=True)
    assert lc.x_p_std[1] == 1.0 and lc.x_p_mean[1] == 4.0
    z = lc._normalize_x(x)
    assert torch.isfinite(z).all() and (z[:, 1] == 0).all()
    assert torch.allclose(z[:, 0].std(), torch.tensor(1.0), atol=1e-5)
    assert torch.allclose(lc._normalize_theta(post).mean(0), torch.zeros(2), atol=1e-5)
    assert torch.equal(LC2ST(th, x, post)._normalize_x(x), x)
    joint = lc._joint(lc.theta_p, lc.theta_q, lc.x_p, lc.x_q)
    assert joint.shape == (100, 5) and torch.equal(joint[:50, 2:], joint[50:, 2:])


def test_null_members_keep_the_label_multiset_and_the_data_rows():
    n = 60
    th_p, th_q = torch.arange(n).float()[:, None], (100 + torch.arange(n)).float()[:, None]
    a, b = permute_data(th_p, th_q, seed=4)
    perm = L._null_permutation(n, 4)
    joint = torch.cat([th_p, th_q])
    assert torch.equal(a, joint[perm[:n]]) and torch.equal(b, joint[perm[n:]])       # the reference's permute_data
    obs = L.build_members(n, 1, 1, 1, [(0, None, 0)])
    null = L.build_members(n, 1, 1, 1, [(1, perm, 0)])
    for mem in (obs, null):
        tot = int(mem.n_train[0] + mem.n_valid[0])
        assert tot == 2 * n and sorted(mem.rows[0, :tot]) == list(range(2 * n))      # every data row exactly once
        assert mem.labels[0, :tot].sum() == n                                         # the label multiset
    lab_obs = dict(zip(obs.rows[0], obs.labels[0]))
    assert all(lab_obs[r] == (r >= n) for r in range(2 * n))
    lab_null = dict(zip(null.rows[0], null.labels[0]))
    assert all(lab_null[perm[j]] == (j >= n) for j in range(2 * n))                  # position in the permuted halves
    assert any(lab_null[r] != lab_obs[r] for r in range(2 * n))


def test_folds_partition_each_half_and_match_sklearn():
    n, k = 23, 4
    folds = L.kfold_train_indices(n, k, seed=3)
    held = [np.setdiff1d(np.arange(n), f) for f in folds]
    assert sorted(np.concatenate(held)) == list(range(n))
    assert sorted(len(h) for h in held) == [5, 6, 6, 6]
    from sklearn.model_selection import KFold

    for mine, (theirs, _) in zip(folds, KFold(n_splits=k, shuffle=True, random_state=3).split(np.zeros((n, 1)))):
        assert np.array_equal(mine, theirs)
    mem = L.build_members(n, k, 2, 3, [(0, None, 0)])
    assert len(mem.n_train) == k * 2
    for f in range(k):
        for e in range(2):
            m = f * 2 + e
            tot = int(mem.n_train[m] + mem.n_valid[m])
            want = np.concatenate([folds[f], n + folds[f]])
            assert sorted(mem.rows[m, :tot]) == sorted(want)                         # the fold, cut on both halves
            assert (mem.labels[m, :tot] == (mem.rows[m, :tot] >= n)).all()
    assert L.kfold_train_indices(7, 1, 0)[0].tolist() == list(range(7))


def test_row_lists_and_validation_split_are_disjoint_and_complete():
    n = 101
    mem = L.build_members(n, 1, 3, 5, [(0, None, 0), (1, None, 2 * n)])
    assert mem.member_id.tolist() == [0, 1, 2, 3, 4, 5] and len(set(mem.init_seed.tolist())) == 6
    for m in range(6):
        nt, nv = int(mem.n_train[m]), int(mem.n_valid[m])
        assert nv == 21 and nt + nv == 2 * n                       # ceil(10 %) held out
        off = 0 if m < 3 else 2 * n
        train, valid = set(mem.rows[m, :nt]), set(mem.rows[m, nt:nt + nv])
        assert not (train & valid) and train | valid == set(range(off, off + 2 * n))
    assert not np.array_equal(mem.rows[0], mem.rows[1])             # a split drawn per member
    again = L.build_members(n, 1, 3, 5, [(0, None, 0), (1, None, 2 * n)])
    assert np.array_equal(mem.rows, again.rows)                     # and a pure function of the seed


def test_initial_weights_follow_nn_linear_defaults():
    h = L.LC2STHyper(3, 4, 20)
    p = L.init_params(h, 9)
    assert p.shape == (h.param_count(),) == (20 * 7 + 400 + 61,)
    w1, b1, w2, b2, w3, b3 = O.split_params(h, p)
    for t, fan_in in ((w1, 7), (b1, 7), (w2, 20), (b2, 20), (w3, 20), (b3, 20)):
        assert t.abs().max() <= fan_in**-0.5
    assert w2.abs().max() > 0.9 * 20**-0.5 and abs(w2.mean()) < 0.02
    assert torch.equal(p, L.init_params(h, 9)) and not torch.equal(p, L.init_params(h, 10))


def test_p_value_from_injected_scores():
    th, x, post = _data()
    lc = LC2ST(th, x, post, num_trials_null=4)
    lc._state = LC2STState.READY
    lc.get_statistic_on_observed_data = lambda theta_o, x_o: 0.3
    lc.get_statistics_under_null_hypothesis = lambda theta_o, x_o, **kw: LC2STScores(np.array([0.1, 0.3, 0.5, 0.7]))
    assert lc.p_value(th, x[0]) == 0.5                # strictly above only
    assert lc.reject_test(th, x[0]) is False and lc.reject_test(th, x[0], alpha=0.6) is True
    lc.get_statistic_on_observed_data = lambda theta_o, x_o: 0.9
    assert lc.p_value(th, x[0]) == 0.0 and lc.reject_test(th, x[0]) is True


def test_refusals_name_the_offending_item():
    th, x, post = _data()
    from sklearn.ensemble import RandomForestClassifier
    from sklearn.neural_network import MLPClassifier

    assert LC2ST(th, x, post, classifier=MLPClassifier).hyper == LC2ST(th, x, post, classifier="MLP").hyper
    assert LC2ST(th, x, post).hyper == L.LC2STHyper(2, 3, 20, 200, 0.01, 1e-4, 0.9, 0.999, 1e-8, 50, 1e-4, 1000)
    ok = LC2ST(th, x, post, classifier_kwargs=dict(module__hidden_layer_sizes=(64, 64), max_epochs=7, batch_size=50,
                                                   lr=0.1, optimizer__weight_decay=0.0, patience=3)).hyper
    assert (ok.H, ok.max_epochs, ok.batch_size, ok.lr, ok.weight_decay, ok.patience) == (64, 7, 50, 0.1, 0.0, 3)
    with pytest.raises(NotImplementedError, match="random_forest"):
        LC2ST(th, x, post, classifier="random_forest")
    with pytest.raises(NotImplementedError, match="RandomForestClassifier"):
        LC2ST(th, x, post, classifier=RandomForestClassifier)
    with pytest.raises(ValueError, match='Invalid classifier: "svm"'):
        LC2ST(th, x, post, classifier="svm")
    with pytest.raises(TypeError, match="must be a string or a subclass"):
        LC2ST(th, x, post, classifier=3)
    with pytest.raises(NotImplementedError, match="optimizer__amsgrad"):
        LC2ST(th, x, post, classifier_kwargs=dict(optimizer__amsgrad=True))
    with pytest.raises(NotImplementedError, match=r"\(20, 30\)"):
        LC2ST(th, x, post, classifier_kwargs=dict(module__hidden_layer_sizes=(20, 30)))
    with pytest.raises(NotImplementedError, match=r"\(20, 20, 20\)"):
        LC2ST(th, x, post, classifier_kwargs=dict(module__hidden_layer_sizes=(20, 20, 20)))
    with pytest.raises(NotImplementedError, match="hidden width 129"):
        LC2ST(th, x, post, classifier_kwargs=dict(module__hidden_layer_sizes=(129, 129)))
    wide = torch.randn(50, 20)
    with pytest.raises(NotImplementedError, match="hidden width 200"):
        LC2ST(wide, x, wide)                                        # the default 10 D leaves the envelope at D = 13
    xl = torch.randn(50, 63)
    with pytest.raises(NotImplementedError, match="65 inputs"):
        LC2ST(th, xl, post)
    # and the library gives the same answers
    lib = _lib.load()
    assert lib.sbi_amd_lc2st_param_count(L.LC2STHyper(2, 62, 128).c_config()) == L.LC2STHyper(2, 62, 128).param_count()
    assert lib.sbi_amd_lc2st_param_count(L.LC2STHyper(2, 63, 20).c_config()) == _lib.E_UNSUPPORTED
    assert lib.sbi_amd_lc2st_param_count(L.LC2STHyper(2, 3, 129).c_config()) == _lib.E_UNSUPPORTED
    assert lib.sbi_amd_lc2st_param_count(L.LC2STHyper(0, 3, 20).c_config()) == _lib.E_BADARG
    assert lib.sbi_amd_lc2st_eval(L.LC2STHyper(2, 3, 20).c_config(), None, None, None, 4, 1, 1, 1, None, None,
                                  None) == _lib.E_BADARG


def test_a_training_seed_reseeds_the_classifiers_but_keeps_the_folds():
    a = L.build_members(40, 3, 1, 1, [(0, None, 0)])
    b = L.build_members(40, 3, 1, 9, [(0, None, 0)], fold_seed=1)      # what train_on_observed_data(seed=9) builds
    c = L.build_members(40, 3, 1, 9, [(0, None, 0)])
    for m in range(3):
        tot = int(a.n_train[m] + a.n_valid[m])
        assert sorted(a.rows[m, :tot]) == sorted(b.rows[m, :tot])               # the same fold ...
        assert not np.array_equal(a.rows[m, :tot], b.rows[m, :tot])             # ... another validation split
    assert any(sorted(a.rows[m, :int(a.n_train[m] + a.n_valid[m])]) != sorted(c.rows[m, :int(c.n_train[m] + c.n_valid[m])])
               for m in range(3))
    assert (a.init_seed != b.init_seed).all()


def test_only_sklearns_own_mlp_class_means_mlp():
    th, x, post = _data()
    from sklearn.base import BaseEstimator

    class MLPClassifier:                      # the name alone is not enough
        pass

    class Mine(BaseEstimator):
        pass

    with pytest.raises(TypeError, match="must be a string or a subclass"):
        LC2ST(th, x, post, classifier=MLPClassifier)
    with pytest.raises(NotImplementedError, match="Mine"):
        LC2ST(th, x, post, classifier=Mine)
    with pytest.raises(ValueError, match="one size"):
        permute_data(th, th[:5])


def test_early_stopping_bookkeeping_on_a_hand_made_sequence():
    seq = [1.0, 0.9, 0.89995, 0.95, 0.8, 0.81, 0.82, 0.83]
    #      best  best  <1e-4: miss  miss  best  miss  miss -> stop (patience 2 would have stopped at epoch 4)
    es = O.EarlyStopper(patience=3, max_epochs=100)
    flags = []
    for v in seq:
        flags.append(es.update(v))
        if es.stopped:
            break
    assert flags == [True, True, False, False, True, False, False, False]
    assert (es.stopped, es.epoch, es.best_epoch, es.best, es.misses) == (True, 8, 4, 0.8, 3)
    assert L.early_stopping_replay(seq, 3, 100) == (True, 8, 4)
    assert L.early_stopping_replay(seq, 2, 100) == (True, 4, 1)
    assert L.early_stopping_replay(seq[:3], 3, 100) == (False, 3, 1)
    # max_epochs ends a run that still improves; NaN never counts as an improvement
    es = O.EarlyStopper(patience=5, max_epochs=3)
    for v in (0.7, 0.6, 0.5):
        es.update(v)
    assert (es.stopped, es.epoch, es.best_epoch) == (True, 3, 2) == L.early_stopping_replay([0.7, 0.6, 0.5], 5, 3)
    assert L.early_stopping_replay([0.7, float("nan"), float("nan")], 2, 9) == (True, 3, 0)


def test_epoch_orders_are_permutations_keyed_by_member_id():
    a = O.epoch_order(37, 5, 0, 7)
    assert sorted(a) == list(range(37))
    assert not np.array_equal(a, O.epoch_order(37, 5, 1, 7)) and not np.array_equal(a, O.epoch_order(37, 5, 0, 8))
    assert not np.array_equal(a, O.epoch_order(37, 6, 0, 7)) and np.array_equal(a, O.epoch_order(37, 5, 0, 7))


def test_header_binding_and_library_agree():
    text = open(os.path.join(ROOT, "include", "sbi_amd_lc2st.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(sbi_amd_\w+)\s*\(", text))
    assert declared == set(_lib.exported_symbols_lc2st()) and len(declared) == 4
    assert not declared & set(_lib.exported_symbols()) and not declared & set(_lib.exported_symbols_npse())
    _build.build()
    lib = ctypes.CDLL(str(_build.LIB_PATH))
    for s in declared:
        assert hasattr(lib, s), s
    # the config struct mirrors the header field for field
    fields = re.search(r"typedef struct sbi_amd_lc2st_config \{(.*?)\}", text, flags=re.S).group(1)
    names = [n.strip() for decl in re.findall(r"(?:int32_t|float)\s+([^;]+);", fields) for n in decl.split(",")]
    assert names == [f[0] for f in _lib.LC2STConfigC._fields_]
