"""Calibration of the fp32 round-off model (tests/fp32_error_model.py) without a GPU, on every mat-vec case shape of
tests/test_gpu_fp32_parity.py:

* an fp32 emulation in torch-CPU float32 (centred Gram form, float32 exp2, sequential chunked accumulation) stays within tau / 4;
* every planted defect exceeds tau * s on at least one entry: the GPU test would see such a kernel bug;
* s is not vacuous: at the median row the emulation's own error is above tau * s / 1000."""
import numpy as np
import pytest

import fp32_error_model as em

TAU = em.TAU["matvec"]


def _shapes():
    out = [(f"matvec-{kind}-D{D}-N{N}" + (f"-c{ch}" if ch else ""), kind, dict(N=N, D=D), ch, 0, None) for kind, D, N, ch in em.matvec_shapes()]
    for D in (8, 24):
        for kind in em.KINDS:
            out += [(f"shard-{kind}-D{D}-{r0}-{r1}", kind, dict(N=2999, D=D, seed=7), 0, r0, r1) for r0, r1 in em.SHARDS]
    for kind in em.KINDS:
        out += [(f"edge-{kind}-{label}", kind, dict(edge=kw), 0, 0, None) for label, kw in em.EDGE_CASES]
    return out


SHAPES = _shapes()


def _case(kind, spec, chunk, r0, r1):
    if "edge" in spec:
        X32, _, hyp, p32 = em.edge_problem(**spec["edge"])
    else:
        X32, _, hyp, p32 = em.problem(**spec)
    case = em.matvec_case(kind, X32, hyp, p32, r0=r0, r1=r1, chunk=chunk or None)
    return X32, hyp, p32, case


@pytest.mark.parametrize("name,kind,spec,chunk,r0,r1", SHAPES, ids=[s[0] for s in SHAPES])
def test_emulation_within_a_quarter_of_tau_and_defects_fire(name, kind, spec, chunk, r0, r1):
    X32, hyp, p32, case = _case(kind, spec, chunk, r0, r1)
    N, D = X32.shape
    emu = em.emulate_matvec(kind, X32, hyp, p32, case.chunk, r0, r1)
    rel = np.abs(emu - case.ref) / case.s
    assert rel.max() <= TAU / 4, f"emulation at {rel.max():.3g} of s, tau / 4 = {TAU / 4}"
    if N > 1:  # (N = 1: one product and a noise term)
        assert np.median(rel) > 1e-3 * TAU, "s is vacuous: the emulation's median error is below tau * s / 1000"
    if N == 1:  # one diagonal entry: no column, no chunk edge, no pair for a lengthscale to act on; the missing noise term only
        assert em.ratio(em.defect_shard_noise(case, p32, r0, hyp.noise), case.ref, case.s) > TAU
        return
    defects = {"drop last column": em.defect_drop_last_column(case, p32),
               "drop a row of the last 64-row group": em.defect_drop_tail_row(case, p32),
               "no noise on the shard's first row": em.defect_shard_noise(case, p32, r0, hyp.noise),
               "a column twice at a chunk edge": em.defect_double_column(case, p32)}
    blunt = {k: em.ratio(v, case.ref, case.s) for k, v in defects.items()}
    assert all(r > TAU for r in blunt.values()), f"planted defects below tau = {TAU}: {blunt}"
    if D <= em.LS_DEFECT_MAX_D and "edge" not in spec:  # (fp32's own resolution limit: fp32_error_model.py docstring)
        r = em.ratio(em.defect_lengthscale(kind, X32, hyp, p32, r0, r1), case.ref, case.s)
        assert r > (TAU if kind == "rbf" else 0.4 * TAU), f"lengthscale 1e-5 off at {r:.3g} of s (tau {TAU})"


def test_dispatch_facts():
    """The launcher rules the model reads: padded widths, rows per lane (8 / 4 / 2 in fp32) and the symmetric kernel's chunk."""
    assert [em.pad_dim(d) for d in (1, 5, 9, 17, 25, 29, 32, 33)] == [1, 6, 10, 20, 28, 32, 32, 33]
    assert [em.rows_per_lane(d) for d in (4, 5, 16, 17, 32)] == [8, 4, 4, 2, 2]
    assert em.sym_chunk(2999, 8) == 128 and em.sym_chunk(2999, 8, opt=100) == 112 and em.sym_chunk(1_000_000, 16) == 1024
    # the fp64 instances (optional dtype argument; the defaults above stay fp32): 8 / 4 up to the padded width 12 / 2 / 1
    assert [em.rows_per_lane(d, "fp64") for d in (3, 4, 5, 8, 12, 13, 16, 17, 20, 32, 50, 96)] == [8, 8, 4, 4, 4, 2, 2, 1, 1, 1, 1, 1]
    assert [em.rows_per_lane(d, "fp32") for d in (3, 16, 24)] == [8, 4, 2]
    # fp64, D = 8 (256-row blocks): 128 columns below ~46k rows, 1024 only above ~93k; the thresholds move with the rows per lane
    assert [em.sym_chunk(n, 8, dtype="fp64") for n in (7000, 45_000, 48_000, 66_000, 92_000, 94_000)] == [128, 128, 256, 512, 512, 1024]
    assert em.sym_chunk(48_000, 8, dtype="fp64") != em.sym_chunk(48_000, 20, dtype="fp64")
    assert em.sym_chunk(94_000, 8, world=8, dtype="fp64") == 128
    assert [em.sym_chunk(3000, 8, opt=o, dtype="fp64") for o in (16, 1000, 1024, 4096)] == [16, 1008, 1024, 1024]
    assert em.quantity("matvec_v2") == "matvec" and em.quantity("cross_n77") == "cross" and em.quantity("f_var") == "f_var"
