"""The restatement of the training-input gradients (tests/train_input_grad_ref.py), checked without a GPU:

* the dense formula against central differences of gpr_ref.lml_only (N = 60, D = 3, step 1e-6; tolerance 1e-6 of the largest entry, measured
  5e-9 .. 2.3e-8);
* the torch lml against gpr_ref.evaluate, value and hyper-parameter gradient, and its autograd input gradient against the dense formula;
* the scaling and translation identities of the pair form;
* every planted defect misses the GPU test's tolerance by 100 times or more on the cells it applies to;
* the mirrors of the launcher's rules against the constants of csrc/row_slab.h and csrc/kernels_train_input_grad.hip, read as text.
"""
import os
import re

import numpy as np
import pytest

import gpr_ref
import matern52_ref as m5
import train_input_grad_ref as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cglb_amd", "csrc")
N, D = 60, 3


def _pairs(n, S, seed=0):
    rng = np.random.default_rng(1000 + seed + n + S)
    return rng.standard_normal((n, S)), rng.standard_normal((n, S))


@pytest.mark.parametrize("trained", [False, True], ids=["init", "trained"])
@pytest.mark.parametrize("kind", tr.KINDS)
def test_dense_formula_matches_central_differences(kind, trained):
    X, y = gpr_ref.problem(N, D)
    h = gpr_ref.hypers(D, trained)
    w, _ = tr.gpr_weight(kind, X, y, h)
    gx = tr.grad_x(kind, X, h["lengthscales"], h["variance"], w=w)[0].astype(np.float64)
    fd = np.empty_like(gx)
    step = 1e-6
    with m5.oracle_with_matern52():
        for i in range(N):
            for k in range(D):
                Xp, Xm = X.copy(), X.copy()
                Xp[i, k] += step
                Xm[i, k] -= step
                fd[i, k] = (gpr_ref.lml_only(kind, Xp, y, **h) - gpr_ref.lml_only(kind, Xm, y, **h)) / (2 * step)
    err = np.abs(gx - fd).max() / np.abs(gx).max()
    print(f"{kind} trained={trained}: {err:.2e} of the largest entry")
    assert err <= 1e-6


@pytest.mark.parametrize("trained", [False, True], ids=["init", "trained"])
@pytest.mark.parametrize("kind", tr.KINDS)
def test_torch_lml_matches_gpr_ref_and_the_dense_formula(kind, trained):
    import torch
    X, y = gpr_ref.problem(N, D)
    h = gpr_ref.hypers(D, trained)
    with m5.oracle_with_matern52():
        ref = gpr_ref.evaluate(kind, X, y, **h)
    x = torch.tensor(X, dtype=torch.float64, requires_grad=True)
    hyp = [torch.tensor(np.asarray(h[k], dtype=np.float64), requires_grad=True) for k in ("lengthscales", "variance", "noise", "mean")]
    lml = tr.torch_lml(kind, x, torch.tensor(y), *hyp)
    lml.backward()
    assert abs(float(lml.detach()) - ref.lml) <= 1e-12 * abs(ref.lml)
    got = np.concatenate([hyp[0].grad.numpy().reshape(-1)] + [t.grad.numpy().reshape(1) for t in hyp[1:]])
    want = gpr_ref.grad_vector(ref.grad)
    assert np.all(np.abs(got - want) <= 1e-9 * np.abs(want).max())
    w, _ = tr.gpr_weight(kind, X, y, h)
    gx = tr.grad_x(kind, X, h["lengthscales"], h["variance"], w=w)[0].astype(np.float64)
    assert np.abs(x.grad.numpy() - gx).max() <= 1e-9 * np.abs(gx).max()


@pytest.mark.parametrize("kind", tr.KINDS)
@pytest.mark.parametrize("S", [1, 9])
def test_scaling_and_translation_identities(kind, S):
    X, _ = gpr_ref.problem(N, D)
    h = gpr_ref.hypers(D, True)
    U, V = _pairs(N, S)
    gx, scale = tr.grad_x(kind, X, h["lengthscales"], h["variance"], U, V)
    Gl, Gabs = tr.lengthscale_forms(kind, X, h["lengthscales"], h["variance"], U, V)
    ls = np.asarray(h["lengthscales"], dtype=tr.LD)
    Xl = np.asarray(X, dtype=tr.LD)
    lhs = (Xl * gx).sum(axis=0)
    assert np.all(np.abs(lhs + ls * Gl) <= 1e-15 * (np.abs(Xl) * scale).sum(axis=0))
    assert np.all(np.abs(gx.sum(axis=0)) <= 1e-15 * scale.sum(axis=0))
    assert np.all(Gabs > 0)


def _defect_cells(defect):
    """(N, D, S, forced jsplit) on which the defect shows"""
    if defect == "drop_groups_after_first":
        return [(63, 3, 9, 0), (63, 20, 5, 0)]
    if defect == "drop_chunk_last":
        return [(257, 3, 2, 3), (130, 12, 9, 7)]
    return [(63, 3, 1, 0), (63, 8, 9, 0)]


@pytest.mark.parametrize("defect", tr.DEFECTS)
@pytest.mark.parametrize("kind", tr.KINDS)
def test_every_defect_misses_the_gpu_tolerance(kind, defect):
    for n, d, S, forced in _defect_cells(defect):
        X, _ = gpr_ref.problem(n, d)
        h = gpr_ref.hypers(d, True)
        U, V = _pairs(n, S)
        good, scale = tr.grad_x(kind, X, h["lengthscales"], h["variance"], U, V)
        _, chunk = tr.split(n, d, forced)
        bad, _ = tr.grad_x(kind, X, h["lengthscales"], h["variance"], U, V, defect=defect, chunk=chunk, group=tr.group_width(d))
        tol = tr.tolerance(scale, np.abs(tr.pair_weights(U, V)).sum(axis=1), h["variance"])
        miss = (np.abs(bad - good).astype(np.float64) / tol).max()
        print(f"{kind} {defect} N={n} D={d} S={S}: misses by {miss:.1e}")
        assert miss >= 100


def test_rule_mirrors_agree_with_the_header():
    text = open(os.path.join(CSRC, "row_slab.h")).read()
    r = re.search(r"train_input_grad_rows_per_lane\(int dp\) \{ return dp <= (\d+) \? (\d+) : (\d+); \}", text)
    g = re.search(r"train_input_grad_group_width\(int dp\) \{ return dp <= (\d+) \? (\d+) : (\d+); \}", text)
    assert r and g
    rcut, rlo, rhi = map(int, r.groups())
    gcut, glo, ghi = map(int, g.groups())
    for d in range(1, 33):
        dp = tr.pad_dim(d)
        assert tr.rows_per_lane(d) == (rlo if dp <= rcut else rhi)
        assert tr.group_width(d) == (glo if dp <= gcut else ghi)
        # the sizing the header states: column side 2 DP + 4 G SGPRs within the 102 of a wave, with room for addresses and the loop
        assert 2 * dp + 4 * tr.group_width(d) <= 80
    src = open(os.path.join(CSRC, "kernels_train_input_grad.hip")).read()
    assert int(re.search(r"#define TRAIN_INPUT_GRAD_ROWS (\d+)", src).group(1)) == tr.ROWS
    assert "kernels_train_input_grad.hip" in open(os.path.join(CSRC, "Makefile")).read()
    dps = [int(m) for m in re.findall(r"case (\d+): \{ constexpr int DP", open(os.path.join(CSRC, "dispatch.h")).read())]
    assert [tr.pad_dim(d) for d in dps] == dps and max(dps) == 32


def test_covering_table_reaches_every_class():
    cells = tr.covering_table()
    classes = {(tr.rows_per_lane(d), tr.group_width(d)) for d in range(1, 33)}
    assert classes == set(tr.CLASSES)
    for (R, G), d in tr.CLASSES.items():
        assert (tr.rows_per_lane(d), tr.group_width(d)) == (R, G)
        mine = [c for c in cells if (tr.rows_per_lane(c[1]), tr.group_width(c[1])) == (R, G)]
        assert {1, G, G + 1, 9, 11} <= {c[2] for c in mine}
        assert any(c[0] == 256 * R + 1 for c in mine)
    assert {1, 2, 63, 1100, tr.ROWS + 1} <= {c[0] for c in cells}
    assert {1, 3, 8, 12, 20, 32} <= {c[1] for c in cells}
    assert {0, 1, 3, 7} <= {c[3] for c in cells}
    assert {c[4] for c in cells} == set(tr.KINDS) and {c[5] for c in cells} == {False, True}
    # a forced split beyond one chunk only where there are columns for it
    assert any(tr.split(c[0], c[1], c[3])[0] > 1 for c in cells)
