"""The launch geometry of the symmetric pair kernels (cglb_amd/csrc/pair_worklist.h), checked without a GPU.

The header is pure integer host code: the column-chunk rule and the order of the work list, i.e. which (group of four row blocks, column
unit) pairs a launch evaluates at all.  tests/host/pair_worklist_check.cpp (own main, no HIP) is compiled against it with the host
compiler behind the Makefile's hipcc, once plainly and once with -fsanitize=address,undefined, and run over the geometries of
tests/geometry_cases.py (the single kernel: unit = column chunk, also dealt cyclically over ranks) and over the spans of the multi-column
kernel (LDS chunks of 512 / 256 / 128 columns).  Every property is asserted on the output of both programs."""
import os
import re
import subprocess

import pytest

import geometry_cases as gc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cglb_amd", "csrc")
XCDS = 8


def _hipcc():
    text = open(os.path.join(CSRC, "Makefile")).read()
    return os.environ.get("HIPCC") or re.search(r"^HIPCC \?= (\S+)", text, re.M).group(1)


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def program(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("pair_worklist") / request.param)
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if request.param == "sanitized" else ["-O2"]
    cmd = [_hipcc(), "-x", "c++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, "-I", CSRC,
           os.path.join(ROOT, "tests", "host", "pair_worklist_check.cpp"), "-o", exe]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr

    def run(commands):
        out = subprocess.run([exe], input="".join(c + "\n" for c in commands), capture_output=True, text=True)
        assert out.returncode == 0 and not out.stderr, out.stderr
        lines = out.stdout.split("\n")[:-1]
        assert len(lines) == len(commands)
        return lines
    return run


def _sym_geometry(n, rbrows, chunk, world, rank):
    """(first unit of every group, number of units) of ensure_sym_items: groups of four of this rank's row blocks, units = chunks."""
    nrb = -(-n // rbrows)
    nlb = len(range(rank, nrb, world))
    return [((rank + 4 * g * world) * rbrows) // chunk for g in range(-(-nlb // 4))], -(-n // chunk)


def _multi_rows_per_lane(dp, sp):
    r = 4 if dp <= 12 else (2 if dp <= 16 else 1)
    while r > 1 and r * (dp + 2 * sp) > 64:
        r //= 2
    return r


def _multi_geometry(n, dp, sp, span_rule):
    """kff_multi_generic / ensure_multi_items: the span is Q LDS chunks of at most 1024 / S_pad columns."""
    rbrows = 64 * _multi_rows_per_lane(dp, sp)
    chunk = min(span_rule, 1024 // sp)
    span = -(-span_rule // chunk) * chunk
    nrb = -(-n // rbrows)
    return [(4 * g * rbrows) // span for g in range(-(-nrb // 4))], -(-n // span), chunk


def _geometries():
    geo = {}
    for _, dtype, D, _, opt, _, _, _ in gc.cells():
        for n in gc.sizes(dtype, D, opt):
            geo[f"sym-{dtype}-D{D}-c{opt}-N{n}"] = _sym_geometry(n, gc.rbrows(dtype, D), gc.eff_chunk(opt), 1, 0)
    for world, rank in ((2, 1), (3, 0), (8, 7)):   # the cyclic deal; N = 1500 has three 512-row blocks: rank 7 of 8 has none
        for n, rb, ch in ((1500, 512, 128), (3077, 128, 1008), (2999, 64, 128)):
            geo[f"sym-w{world}r{rank}-N{n}-rb{rb}-c{ch}"] = _sym_geometry(n, rb, ch, world, rank)
    lds = set()
    for dp, sp in ((3, 2), (8, 4), (16, 8), (20, 8), (32, 2)):
        for rule in (16, 128, 320, 512, 1024):   # 320 at S_pad 8: a span that is no multiple of the LDS chunk before it is rounded up
            for n in (1333, 2500):
                first, nunits, chunk = _multi_geometry(n, dp, sp, rule)
                geo[f"multi-Dp{dp}-S{sp}-span{rule}-N{n}"] = (first, nunits)
                lds.add(chunk)
    assert {512, 256, 128} <= lds
    geo["empty"] = ([], 0)
    geo["no-groups"] = ([], 5)
    return geo


def _parse(line):
    v = [int(x) for x in line.split()]
    assert len(v) % 2 == 0
    return list(zip(v[0::2], v[1::2]))


def test_work_order_lists_every_reached_unit_once_in_both_orders(program):
    geo = _geometries()
    assert any(len(first) > 1 and nunits > 2 for first, nunits in geo.values())
    names = [(name, order) for name in geo for order in (0, 1)]
    lines = program([f"order {len(geo[name][0])} {geo[name][1]} {order} " + " ".join(map(str, geo[name][0])) for name, order in names])
    for (name, order), line in zip(names, lines):
        first, nunits = geo[name]
        got = _parse(line)
        group_major = [(g, k) for g, f in enumerate(first) for k in range(f, nunits)]
        valid = [e for e in got if e != (-1, -1)]
        # every (group, unit) the group's first block reaches exactly once; everything else is padding
        assert sorted(valid) == group_major, name
        if not group_major:
            assert got == [(-1, -1)], name           # an empty problem: one padding entry
            continue
        if order == 0:
            assert got == group_major, name
            continue
        assert len(got) % XCDS == 0, name
        by_unit = sorted(group_major, key=lambda e: (e[1], e[0]))
        per = -(-len(by_unit) // XCDS)
        for x in range(XCDS):
            mine = sorted(by_unit[x * per:(x + 1) * per])   # range x of the unit-sorted list, group by group (units ascending inside a group)
            assert got[x::XCDS] == mine + [(-1, -1)] * (per - len(mine)), (name, x)


def test_column_chunk_rule(program):
    def chunk(n, rbrows, world=1, opt=0):
        return int(program([f"chunk {n} {rbrows} {world} {opt}"])[0])
    # a forced chunk: rounded up to 16, clamped to 1024
    assert [chunk(3000, 256, opt=o) for o in (16, 1000, 1024, 5000, 4096, 1, 100)] == [16, 1008, 1024, 1024, 1024, 16, 112]
    # the default rule: 1024, halved down to 128 while a rank has fewer than 16k items (256-row blocks: fp64, D = 8)
    assert [chunk(n, 256) for n in (1, 7000, 45_000, 48_000, 66_000, 92_000, 94_000, 1_000_000)] == [128, 128, 128, 256, 512, 512, 1024, 1024]
    assert chunk(48_000, 256) != chunk(48_000, 64)                      # the rows-per-lane class enters
    assert chunk(94_000, 256, world=8) == 128 and chunk(2999, 256, world=3) == 128
    assert [chunk(3000, 256, opt=o) for o in (0, -1, -2 ** 40)] == [128] * 3     # 0 or negative: the default rule
    # the largest values cglb_set_option lets through clamp without wrapping; the refusal above 2^20 stays in cglb_set_option
    assert [chunk(3000, 256, opt=o) for o in (2 ** 20 - 1, 2 ** 20)] == [1024, 1024]
    api = open(os.path.join(CSRC, "cglb_api.hip")).read()
    option = api[api.index('!strcmp(name, "sym_chunk")'):api.index('!strcmp(name, "sym_order")')]
    assert "value > ((int64_t)1 << 20)" in option and "CGLB_ERR_BAD_ARG" in option
    assert "1 << 20" not in open(os.path.join(CSRC, "pair_worklist.h")).read()
