"""The Matern-5/2 reference of tests/matern52_ref.py and the host layers of the new kind (no GPU).

The closed form is pinned to the general Matern form with a Bessel function, the gradient factor to finite differences, the patched
oracle's analytic gradient to finite differences of its own bound.  `test_matern32_*` show that every reference quantity the GPU tests
compare with separates Matern-5/2 from a kernel that fell through to the Matern-3/2 formula by at least 100 times the tolerance used."""
import math

import numpy as np
import pytest

import matern52_ref as m52
from oracle import cglb_oracle as orc


def test_closed_form_equals_the_bessel_form():
    from scipy.special import gamma, kv
    z = np.geomspace(0.002, 67.0, 4000)      # z = sqrt(2 nu) r
    nu = 2.5
    general = 2.0 ** (1.0 - nu) / gamma(nu) * z ** nu * kv(nu, z)
    closed = m52.k52((z / m52.SQRT5) ** 2, 1.0)
    assert np.abs(closed / general - 1.0).max() <= 1e-13


def test_grad_factor_equals_central_differences_in_the_lengthscale():
    rng = np.random.default_rng(0)
    x1, x2 = rng.standard_normal((50, 3)), rng.standard_normal((50, 3))
    ls, var = np.array([0.7, 1.3, 2.1]), 1.7

    def k(lsv):
        return m52.k52((((x1 - x2) / lsv) ** 2).sum(1), var)

    delta = (x1 - x2) / ls
    h = m52.h52((delta ** 2).sum(1), var)
    for d in range(3):
        e = np.zeros(3)
        e[d] = 1e-6 * ls[d]
        fd = (k(ls + e) - k(ls - e)) / (2 * e[d])
        np.testing.assert_allclose(h * delta[:, d] ** 2 / ls[d], fd, rtol=1e-7, atol=1e-10)
    # h is finite at r = 0: 5 f / 3
    assert m52.h52(np.zeros(1), var)[0] == pytest.approx(5.0 * var / 3.0, rel=1e-15)


def _fd_problem():
    X, y, Z = orc.synthetic_problem(120, 3, 6, seed=4)
    hyp = orc.Hypers(np.array([0.9, 1.4, 2.0]), 1.3, 0.2, 0.1, Z, 1e-6)
    v = 0.1 * np.random.default_rng(1).standard_normal(120)
    return X, y, hyp, v


def test_patched_oracle_gradient_equals_central_differences_of_its_bound():
    X, y, hyp, v = _fd_problem()
    with m52.oracle_with_matern52():
        g = orc.objective(m52.KIND, X, y, hyp, v, run_cg=False, with_grad=True).grad

        def bound(h):
            return orc.objective(m52.KIND, X, y, h, v, run_cg=False).bound

        def fd(setter, n, step):
            out = np.zeros(n)
            for i in range(n):
                hp, hm = hyp.copy(), hyp.copy()
                setter(hp, i, step)
                setter(hm, i, -step)
                out[i] = (bound(hp) - bound(hm)) / (2 * step)
            return out

        def set_ls(h, i, s): h.lengthscales[i] += s
        def set_var(h, i, s): h.variance += s
        def set_noise(h, i, s): h.noise += s
        def set_mean(h, i, s): h.mean += s
        def set_z(h, i, s): h.Z.reshape(-1)[i] += s

        blocks = {"lengthscales": fd(set_ls, 3, 1e-6), "variance": fd(set_var, 1, 1e-6), "noise": fd(set_noise, 1, 1e-7),
                  "mean": fd(set_mean, 1, 1e-6), "Z": fd(set_z, hyp.Z.size, 1e-6)}
    for key, num in blocks.items():
        ana = np.asarray(g[key], dtype=np.float64).reshape(-1)
        assert np.abs(ana - num).max() <= 1e-6 * np.abs(num).max(), key


def test_kernel_matrix_is_positive_semi_definite_with_unit_diagonal():
    rng = np.random.default_rng(2)
    X = rng.standard_normal((200, 4))
    X[17] = X[3]
    X[150] = X[3]
    with m52.oracle_with_matern52():
        K = orc.kernel_matrix(m52.KIND, X, X, np.array([0.8, 1.0, 1.5, 2.0]), 1.9)
    assert np.array_equal(np.diag(K), np.full(200, 1.9))
    assert K[3, 17] == 1.9 and K[17, 150] == 1.9
    assert np.linalg.eigvalsh(K).min() >= -1e-12 * 200 * 1.9


def test_the_oracle_is_restored_on_exit_and_on_exceptions():
    before = (orc.kernel_from_sqdist, orc.kernel_grad_factor, orc.KINDS, dict(orc.KINDS))
    with m52.oracle_with_matern52():
        assert orc.kind_id("matern52") == 2 and orc.kernel_from_sqdist is not before[0]
        # other kinds go to the originals
        d2 = np.array([0.0, 0.3, 4.0])
        assert np.array_equal(orc.kernel_from_sqdist("matern32", d2, 1.1), before[0]("matern32", d2, 1.1))
        assert np.array_equal(orc.kernel_grad_factor("rbf", d2, 1.1), before[1]("rbf", d2, 1.1))
    with pytest.raises(RuntimeError):
        with m52.oracle_with_matern52():
            raise RuntimeError("inside")
    assert orc.kernel_from_sqdist is before[0] and orc.kernel_grad_factor is before[1] and orc.KINDS is before[2] and orc.KINDS == before[3]
    with pytest.raises(KeyError):
        orc.kind_id("matern52")


def test_max_distance_between_the_two_matern_profiles():
    r = np.linspace(0.0, 10.0, 100001)
    assert np.abs(m52.k52(r * r, 1.0) - m52.k32(r * r, 1.0)).max() == pytest.approx(0.049, abs=1e-3)


def test_matern32_profile_or_grad_factor_misses_every_gpu_tolerance_by_100x():
    """What tests/test_gpu_matern52.py compares with, evaluated with the Matern-3/2 profile (or with the 3/2 gradient factor alone) in
    place of the 5/2 one: each differs from the true reference by >= 100 times that test's tolerance."""
    import geometry_cases as gc
    X, y, Z = orc.synthetic_problem(300, 3, 12, seed=11)
    hyp = orc.trained_like_hypers(3, Z)
    p = np.random.default_rng(3).standard_normal(300)
    # mat-vec: |out - ref| <= ATOL64 max|ref|
    ref, wrong = m52.dense_matvec(X, hyp, p), m52.dense_matvec(X, hyp, p, profile=m52.k32)
    assert np.abs(wrong - ref).max() >= 100 * gc.ATOL64 * np.abs(ref).max()
    v = np.zeros(300)
    with m52.oracle_with_matern52():
        good = orc.objective(m52.KIND, X, y, hyp, v, True, 1.0, with_grad=True)
        fm, fv, _, _ = orc.predict(m52.KIND, X, y, hyp, v, X[:20] + 0.1)
    with m52.oracle_with_matern52(profile=m52.k32, grad_factor=m52.h32):
        bad = orc.objective(m52.KIND, X, y, hyp, v, True, 1.0, with_grad=True)
        fm3, fv3, _, _ = orc.predict(m52.KIND, X, y, hyp, v, X[:20] + 0.1)
    with m52.oracle_with_matern52(grad_factor=m52.h32):      # right values, 3/2 gradient factor
        badh = orc.objective(m52.KIND, X, y, hyp, good.v, False, with_grad=True)
    assert abs(bad.bound - good.bound) >= 100 * 1e-9 * abs(good.bound)          # bound to 1e-9 relative
    assert abs(bad.logdet - good.logdet) >= 100 * 1e-10 * abs(good.logdet)      # log-det to 1e-10
    for key in ("lengthscales", "Z"):                                           # blocks to rtol 1e-7, atol 1e-8 max
        g = np.asarray(good.grad[key])
        for other in (bad, badh):
            assert np.abs(np.asarray(other.grad[key]) - g).max() >= 100 * (1e-7 * np.abs(g).max() + 1e-8 * max(1.0, np.abs(g).max())), key
    assert np.abs(fm3 - fm).max() >= 100 * 1e-6 * np.abs(fm).max() and np.abs(fv3 - fv).max() >= 100 * 1e-6 * np.abs(fv).max()


def test_fp32_error_model_envelope_covers_matern52_within_14_percent():
    """fp32_error_model's Gram envelope of the non-RBF kinds, E = 3/2 f exp(-sqrt3 r), is written inline there.  The true Matern-5/2
    envelope |dk/d(d^2)| = 5/6 f (1 + sqrt5 r) exp(-sqrt5 r) exceeds it by at most 1.14 (1.136 at r = 1.54) - inside the 4x margin of
    the model's TAU, which is why the fp32 GPU tests use the model unchanged."""
    r = np.linspace(0.0, 40.0, 400001)
    true = 5.0 / 6.0 * (1.0 + m52.SQRT5 * r) * np.exp(-m52.SQRT5 * r)
    model = 1.5 * np.exp(-math.sqrt(3.0) * r)
    ratio = true / model
    assert ratio.max() <= 1.14
    assert r[np.argmax(ratio)] == pytest.approx(1.54, abs=0.02) and ratio.max() == pytest.approx(1.136, abs=2e-3)
    # the envelope really is the derivative of the profile
    d2 = np.linspace(0.01, 9.0, 1000)
    fdiff = (m52.k52(d2 + 1e-6, 1.0) - m52.k52(d2 - 1e-6, 1.0)) / 2e-6
    np.testing.assert_allclose(-fdiff, 5.0 / 6.0 * (1.0 + m52.SQRT5 * np.sqrt(d2)) * np.exp(-m52.SQRT5 * np.sqrt(d2)), rtol=1e-6)


# --------------------------------------------------------------------------- host layers
def test_config_and_registries():
    from cglb_amd.backend import config as cfg
    data = (np.zeros((5, 4)), np.zeros(5))
    params = cfg.Matern52Config().params(data)
    assert params["variance"] == 1.0 and np.array_equal(params["lengthscales"], np.ones(4))
    assert not isinstance(cfg.Matern52Config(), cfg.Matern32Config) and isinstance(cfg.Matern52Config(), cfg.SquaredExponentialConfig)
    assert set(cfg.KERNEL_CONFIGS) == {"SquaredExponential", "Matern32", "mat32", "rbf"}
    assert cfg.EXTRA_KERNEL_CONFIGS == {"Matern52": cfg.Matern52Config, "mat52": cfg.Matern52Config}
    assert "Matern52Config" in cfg.__all__ and "EXTRA_KERNEL_CONFIGS" in cfg.__all__
    import cglb_amd.backend as backend
    assert backend.Matern52Config is cfg.Matern52Config and backend.EXTRA_KERNEL_CONFIGS is cfg.EXTRA_KERNEL_CONFIGS


def test_kind_tables():
    from cglb_amd import _lib
    from cglb_amd.hip_context import KINDS
    assert _lib.MATERN52 == 2
    assert KINDS["matern52"] == KINDS["Matern52"] == KINDS["mat52"] == KINDS[2] == 2
    assert KINDS["matern32"] == 1 and KINDS["rbf"] == 0


def test_create_kernel_and_numpy_closed_form():
    from cglb_amd.backend import config as cfg
    from cglb_amd.backend import interface
    rng = np.random.default_rng(5)
    X = rng.standard_normal((40, 3))
    data = (X, np.zeros(40))
    kernel = interface.create_kernel(cfg.Matern52Config(), data)
    assert kernel.base_kernel.kind == "matern52"
    assert interface.create_kernel(cfg.Matern32Config(), data).base_kernel.kind == "matern32"
    assert interface.create_kernel(cfg.SquaredExponentialConfig(), data).base_kernel.kind == "rbf"
    kernel.base_kernel.lengthscale = np.array([0.7, 1.1, 1.9])
    kernel.outputscale = 1.3
    K = interface._kernel_numpy(kernel, X, X[:7], True)
    ref = m52.k52(orc.scaled_sqdist(X, X[:7], np.array([0.7, 1.1, 1.9])), 1.3)
    np.testing.assert_allclose(K, ref, rtol=0, atol=1e-13)
    assert np.abs(K - m52.k32(orc.scaled_sqdist(X, X[:7], np.array([0.7, 1.1, 1.9])), 1.3)).max() > 1e-2
    assert np.array_equal(interface._kernel_numpy(kernel, X, None, False), np.full(40, 1.3))
    kernel.base_kernel.kind = "periodic"
    with pytest.raises(ValueError, match="periodic"):
        interface._kernel_numpy(kernel, X, X, True)


@pytest.mark.parametrize("group,command", [("train", "cglb"), ("train", "sgpr"), ("train", "gpr"), ("metric", "cglb")])
def test_cli_lists_the_new_kernel(monkeypatch, tmp_path, group, command):
    from click.testing import CliRunner
    from cglb_amd import cli as cli_mod
    from cglb_amd.backend import interface
    monkeypatch.setattr(interface, "configure_backend", lambda **kw: None)  # no HIP device here: --help reaches no GPU
    res = CliRunner().invoke(cli_mod.main, ["-l", str(tmp_path), group, "-d", "synthetic-300-3", command, "--help"])
    assert res.exit_code == 0, res.output
    assert "Matern52" in res.output and "mat52" in res.output and "Matern32" in res.output
