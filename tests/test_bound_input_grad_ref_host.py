"""The restatement of the training-input gradient of the CGLB / SGPR bounds (tests/bound_input_grad_ref.py), checked without a GPU:

* the np.longdouble products of the restated adjoints, gx_kuf + gx_kff, against torch autograd of bound_variants_ref.bound in X (N = 60, D = 3,
  every class and kind).  Tolerance 1e-10 of the largest entry: both sides are dense fp64 evaluations through the Cholesky factors of K_uu and
  B, whose conditioning (below 1e5 here) times 2^-53 bounds the difference of two fp64 routes; measured 3e-14 .. 4e-13;
* the same products against central differences of the bound in X (step 1e-6; tolerance 1e-6 of the largest entry: truncation h^2 |b'''| / 6 and
  round-off 2^-53 |b| / h are both near 1e-8 of it; measured below 1e-7);
* each planted defect misses the tolerance of the GPU test (1e-11 of the per-element sum of absolute terms for the panel pass,
  train_input_grad_ref.tolerance for the pair pass) by a factor of 1e6 or more on the cells it applies to;
* the mirrors of the launcher's rules against csrc/row_slab.h and csrc/kernels_train_input_grad.hip, read as text, and the covering tables.
"""
import os
import re

import numpy as np
import pytest

import bound_input_grad_ref as br
import train_input_grad_ref as tr
from cglb_amd.data import synthetic_problem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cglb_amd", "csrc")
N, M, D = 60, 8, 3


def _problem(trained):
    X, y, Z = synthetic_problem(N, D, M, seed=1)
    h = dict(lengthscales=np.full(D, 1.5), variance=1.0, noise=0.05, mean=0.1) if trained else \
        dict(lengthscales=np.ones(D), variance=1.0, noise=1.0, mean=0.0)
    v = 0.3 * np.random.default_rng(0).standard_normal(N)
    return X, y, Z, h, v


@pytest.mark.parametrize("trained", [False, True], ids=["init", "trained"])
@pytest.mark.parametrize("kind", br.KINDS)
@pytest.mark.parametrize("cls", br.CLASSES)
def test_products_of_the_adjoints_match_torch_autograd(cls, kind, trained):
    X, y, Z, h, v = _problem(trained)
    vv = None if br.OPTIONS[cls][1] else v
    _, gx_ref, _ = br.bound_and_grad_x(cls, kind, X, y, h, Z, v=vv)
    gx, scale = br.bound_grad_x(cls, kind, X, y, h, Z, v=vv)
    err = np.abs(gx.astype(np.float64) - gx_ref).max() / np.abs(gx_ref).max()
    print(f"{cls} {kind} trained={trained}: {err:.2e} of the largest entry {np.abs(gx_ref).max():.3g}")
    assert err <= 1e-10
    assert np.all(scale > 0)


@pytest.mark.parametrize("kind", br.KINDS)
@pytest.mark.parametrize("cls", br.CLASSES)
def test_products_of_the_adjoints_match_central_differences(cls, kind):
    import torch

    import matern52_ref as m5
    X, y, Z, h, v = _problem(True)
    vv = None if br.OPTIONS[cls][1] else v
    gx = br.bound_grad_x(cls, kind, X, y, h, Z, v=vv)[0].astype(np.float64)
    t = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64))
    args = (t(y), t(h["lengthscales"]), t(h["variance"]), t(h["noise"]), t(h["mean"]), t(Z))
    step, fd = 1e-6, np.empty_like(gx)
    with m5.bound_variants_with_matern52() as bref, torch.no_grad():
        value = lambda Xq: float(bref.bound(cls, kind, t(Xq), *args, jitter=1e-6, v=None if vv is None else t(vv)))
        for i in range(N):
            for k in range(D):
                Xp, Xm = X.copy(), X.copy()
                Xp[i, k] += step
                Xm[i, k] -= step
                fd[i, k] = (value(Xp) - value(Xm)) / (2 * step)
    err = np.abs(gx - fd).max() / np.abs(gx).max()
    print(f"{cls} {kind}: {err:.2e} of the largest entry")
    assert err <= 1e-6


def _panel_operands(n, m, seed=0):
    rng = np.random.default_rng(100 + seed + n + m)
    return rng.standard_normal((m, n)), rng.standard_normal(m), rng.standard_normal(n)


@pytest.mark.parametrize("defect", [d for d in br.DEFECTS if d != "no_transposed_term"])
@pytest.mark.parametrize("kind", br.KINDS)
def test_every_panel_defect_misses_the_gpu_tolerance(kind, defect):
    cells = [(63, 63, 3, 0), (63, 63, 8, 0)] if defect == "G_transposed" else \
        ([(257, 130, 3, 7), (63, 16, 12, 3)] if defect == "drop_chunk_last" else [(63, 16, 3, 0), (63, 130, 8, 0)])
    for n, m, d, forced in cells:
        X = synthetic_problem(n, d, 1, seed=n + d)[0]
        Z = np.random.default_rng(n + m + d).standard_normal((m, d))   # M may exceed N
        ls, var = np.full(d, 1.5), 1.3
        G, c, w = _panel_operands(n, m)
        good, scale = br.kuf_grad_x(kind, X, Z, ls, var, G, c, w)
        _, chunk = br.kuf_split(n, m, d, forced)
        bad, _ = br.kuf_grad_x(kind, X, Z, ls, var, G, c, w, defect=defect, chunk=chunk)
        miss = (np.abs(bad - good).astype(np.float64) / (br.TOL * scale.astype(np.float64))).max()
        print(f"{kind} {defect} N={n} M={m} D={d}: misses by {miss:.1e}")
        assert miss >= 1e6


@pytest.mark.parametrize("kind", br.KINDS)
def test_the_dropped_transposed_term_misses_the_gpu_tolerance(kind):
    n, d = 63, 3
    X, _, _ = synthetic_problem(n, d, 1, seed=5)
    rng = np.random.default_rng(7)
    u, v = rng.standard_normal(n), rng.standard_normal(n)
    ls, var = np.full(d, 1.5), 1.3
    good, scale = br.kff_pair_grad_x(kind, X, ls, var, u, v)
    bad, _ = br.kff_pair_grad_x(kind, X, ls, var, u, v, defect="no_transposed_term")
    tol = tr.tolerance(scale, np.abs(tr.pair_weights(u.reshape(-1, 1), v.reshape(-1, 1))).sum(axis=1), var)
    miss = (np.abs(bad - good).astype(np.float64) / tol).max()
    print(f"{kind}: misses by {miss:.1e}")
    assert miss >= 1e6


def test_rule_mirrors_agree_with_the_sources():
    text = open(os.path.join(CSRC, "row_slab.h")).read()
    r = re.search(r"grad_x_kuf_rows_per_lane\(int dp\) \{ return dp <= (\d+) \? (\d+) : (\d+); \}", text)
    p = re.search(r"train_input_grad_pair_rows_per_lane\(int dp\) \{ return dp <= (\d+) \? (\d+) : \(dp <= (\d+) \? (\d+) : (\d+)\); \}", text)
    assert r and p
    rcut, rlo, rhi = map(int, r.groups())
    c1, v1, c2, v2, v3 = map(int, p.groups())
    for d in range(1, 33):
        dp = tr.pad_dim(d)
        assert br.kuf_rows_per_lane(d) == (rlo if dp <= rcut else rhi)
        assert br.pair_rows_per_lane(d) == (v1 if dp <= c1 else (v2 if dp <= c2 else v3))
    assert int(re.search(r"#define GRAD_X_KUF_TARGET_WG (\d+)", text).group(1)) == br.KUF_TARGET_WG
    assert int(re.search(r"#define GRAD_X_KUF_MIN_CHUNK (\d+)", text).group(1)) == br.KUF_MIN_CHUNK
    rule = text[text.index("static inline void row_slab_panel_split"):]
    rule = rule[:rule.index("\n}\n")]
    for piece in ("forced > 0 ? 1 : GRAD_X_KUF_MIN_CHUNK", "(GRAD_X_KUF_TARGET_WG + row_blocks - 1) / row_blocks", "if (msplit > slot_cap) msplit = slot_cap;",
                  "(M + min_chunk - 1) / min_chunk", "(M + msplit - 1) / msplit", "(M + mchunk - 1) / mchunk"):
        assert piece in rule, piece
    src = open(os.path.join(CSRC, "kernels_train_input_grad.hip")).read()
    assert "TRAIN_INPUT_GRAD_ROWS * (train_input_grad_pair_rows_per_lane(dp) > 2 ? 2 : 1)" in src
    assert br.pair_launch_rows(8) == 2 * tr.ROWS and br.pair_launch_rows(12) == tr.ROWS


def test_panel_split_covers_the_inducing_points():
    for forced in (0, 1, 3, 7, 1000):
        for bx in (1, 3, 196, 5000):
            for m in (1, 15, 16, 17, 130, 1024):
                for cap in (1, 20, 256):
                    chunks, chunk = br.panel_split(forced, bx, m, cap)
                    assert 1 <= chunks <= cap and chunks * chunk >= m > (chunks - 1) * chunk
                    if forced:
                        assert chunks <= forced
                    else:
                        assert chunks == 1 or 2 * chunk > br.KUF_MIN_CHUNK   # ceil(M / ceil(M / 16)) > 16 M / (M + 16) >= 8
    assert br.panel_split(0, 196, 1024, 20) == (11, 94)      # N = 100 000 at two rows per lane: 2156 workgroups
    assert br.panel_split(0, 5000, 1024, 256) == (1, 1024)   # row blocks alone fill the device: one chunk
    assert br.panel_split(7, 1, 130, 256) == (7, 19) and br.panel_split(3, 1, 16, 256) == (3, 6) and br.panel_split(3, 1, 1, 256) == (1, 1)


def test_covering_tables_reach_every_class():
    kc, pc = br.kuf_cells(), br.pair_cells()
    assert {br.kuf_rows_per_lane(d) for d in range(1, 33)} == set(br.KUF_CLASSES)
    assert {br.pair_rows_per_lane(d) for d in range(1, 33)} == set(br.PAIR_CLASSES)
    for R, d in br.KUF_CLASSES.items():
        assert br.kuf_rows_per_lane(d) == R
        mine = [c for c in kc if br.kuf_rows_per_lane(c["D"]) == R and c["N"] == 256 * R + 1]
        assert {c["M"] for c in mine} == {1, 16, 130} and {1, 3, 7} <= {c["msplit"] for c in mine}
    assert any(c["pad"] > 0 for c in kc) and any(not c["rank_one"] for c in kc) and any(c["N"] == 4097 for c in kc)
    assert {c["kind"] for c in kc} == set(br.KINDS) and {c["trained"] for c in kc} == {False, True}
    assert any(br.kuf_split(c["N"], c["M"], c["D"], c["msplit"])[0] > 1 for c in kc)
    for R, d in br.PAIR_CLASSES.items():
        assert br.pair_rows_per_lane(d) == R
        assert {1, 3, 7} <= {c[2] for c in pc if c[1] == d and c[0] == 256 * R + 1}
    assert any(c[0] == br.pair_launch_rows(c[1]) + 1 for c in pc)
