"""The host half of the iterative exact-GP estimator (cglb_amd/csrc/slq_host.h), checked without a GPU.

The header is plain C++: the truncation rule of the CG coefficient logs, the Lanczos tridiagonal built from them and the implicit-QL
quadrature e_1^T log(T) e_1.  tests/host/slq_check.cpp (own main, no HIP) is compiled against it with the host compiler behind the
Makefile's hipcc, once plainly and once with -fsanitize=address,undefined; every property is asserted on the output of both programs,
against numpy.linalg.eigh and the numpy restatement of tests/itergp_ref.py."""
import os
import re
import subprocess

import numpy as np
import pytest

import itergp_ref as iref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cglb_amd", "csrc")


def _hipcc():
    text = open(os.path.join(CSRC, "Makefile")).read()
    return os.environ.get("HIPCC") or re.search(r"^HIPCC \?= (\S+)", text, re.M).group(1)


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def program(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("slq") / request.param)
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if request.param == "sanitized" else ["-O2"]
    cmd = [_hipcc(), "-x", "c++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, "-I", CSRC,
           os.path.join(ROOT, "tests", "host", "slq_check.cpp"), "-o", exe]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr

    def run(commands):
        out = subprocess.run([exe], input="".join(c + "\n" for c in commands), capture_output=True, text=True)
        assert out.returncode == 0 and not out.stderr, out.stderr
        lines = out.stdout.split("\n")[:-1]
        assert len(lines) == len(commands)
        return lines
    return run


def _fmt(values):
    return " ".join(repr(float(v)) for v in np.asarray(values, dtype=np.float64).reshape(-1))


def _spd_tridiagonal(n, rng, off_scale=1.0):
    """Diagonally dominant, hence positive definite; eigenvalues spread over about two decades."""
    off = off_scale * rng.uniform(0.1, 1.0, max(n - 1, 0))
    diag = rng.uniform(0.05, 5.0, n)
    diag[:n - 1] += np.abs(off)
    diag[1:] += np.abs(off)
    return diag, off


def _want(diag, off):
    T = np.diag(diag) + np.diag(off, 1) + np.diag(off, -1)
    lam, V = np.linalg.eigh(T)
    terms = V[0] ** 2 * np.log(lam)
    return float(terms.sum()), float(np.abs(terms).sum())


@pytest.mark.parametrize("n", [1, 2, 3, 20, 200])
def test_quadrature_matches_eigh(program, n):
    rng = np.random.default_rng(100 + n)
    cases = [_spd_tridiagonal(n, rng) for _ in range(5)]
    lines = program([f"quad {n} {_fmt(d)} {_fmt(e)}".rstrip() for d, e in cases])
    for (d, e), line in zip(cases, lines):
        status, got = line.split()
        want, scale = _want(d, e)
        print(f"n={n}: {float(got)!r} vs {want!r}: {abs(float(got) - want) / scale:.2e}")
        assert status == "0"
        assert abs(float(got) - want) <= 1e-12 * scale


def test_quadrature_with_a_tiny_off_diagonal(program):
    rng = np.random.default_rng(7)
    d, e = _spd_tridiagonal(20, rng)
    e[9] = 1e-12
    status, got = program([f"quad 20 {_fmt(d)} {_fmt(e)}"])[0].split()
    want, scale = _want(d, e)
    assert status == "0" and abs(float(got) - want) <= 1e-12 * scale


def test_an_eigenvalue_that_is_not_positive_is_reported(program):
    status, _ = program(["quad 2 1.0 1.0 2.0"])[0].split()      # eigenvalues -1 and 3
    assert status == "2"


def _logs(S, t, rng):
    rz = rng.uniform(0.5, 2.0, (S + 1, 1 + t)) * (0.5 ** np.arange(S + 1))[:, None]
    pap = rng.uniform(0.5, 2.0, (S, 1 + t))
    return rz, pap


def test_truncation_rule(program):
    rng = np.random.default_rng(3)
    S, t = 6, 2
    rz, pap = _logs(S, t, rng)

    def steps(rz, pap, col, L):
        got = int(program([f"steps {S} {t} {col} {L} {_fmt(rz)} {_fmt(pap)}"])[0])
        assert got == iref.usable_steps(rz, pap, col, L)
        return got
    assert steps(rz, pap, 1, 20) == S and steps(rz, pap, 1, 4) == 4 and steps(rz, pap, 2, 0) == 0
    for bad in (0.0, float("nan"), float("inf")):
        r2, p2 = rz.copy(), pap.copy()
        r2[3, 1] = bad                       # rz_3 of column 1: steps 0 .. 2 remain; column 2 is untouched
        assert steps(r2, p2, 1, 20) == 3 and steps(r2, p2, 2, 20) == S
        r2, p2 = rz.copy(), pap.copy()
        p2[2, 2] = bad                       # pAp_2 of column 2: gamma_2 is infinite, NaN or zero
        assert steps(r2, p2, 2, 20) == 2 and steps(r2, p2, 1, 20) == S
    r2 = rz.copy()
    r2[0, 1] = 0.0                           # a zero probe: no step at all
    assert steps(r2, pap, 1, 20) == 0


def test_tridiagonal_and_correction_match_the_restatement(program):
    rng = np.random.default_rng(11)
    S, t = 7, 3
    rz, pap = _logs(S, t, rng)
    # make the coefficient logs those of a real CG run so that every T is positive definite: a random SPD matrix and random probes
    n = 30
    Q = rng.standard_normal((n, n))
    Amat = Q @ Q.T + n * np.eye(n)
    B = rng.standard_normal((n, 1 + t))
    _V, steps, _h, rz, pap = iref.batched_pcg(lambda M: Amat @ M, lambda R: R.copy(), B, np.zeros_like(B), 0.0, S)
    assert steps == S
    for col in (1, 3):
        d, e = iref.tridiagonal(rz, pap, col, 5)
        got = np.array([float(x) for x in program([f"tri {S} {t} {col} 5 {_fmt(rz)} {_fmt(pap)}"])[0].split()])
        np.testing.assert_allclose(got[:5], d, rtol=1e-14)
        np.testing.assert_allclose(got[5:], e, rtol=1e-14, atol=0.0)
    for L in (3, 20):
        status, got = program([f"corr {S} {t} {L} {_fmt(rz)} {_fmt(pap)}"])[0].split()
        want = iref.logdet_correction(rz, pap, L)
        scale = 0.0
        for i in range(1, t + 1):
            d, e = iref.tridiagonal(rz, pap, i, iref.usable_steps(rz, pap, i, L))
            scale += rz[0, i] * _want(d, e[:len(d) - 1])[1] / t
        assert status == "0" and abs(float(got) - want) <= 1e-12 * scale
