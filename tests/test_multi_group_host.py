"""The group-width rule of the multi-column K_ff product (cglb_amd/csrc/pair_worklist.h: multi_mid_group, multi_mid_partials,
multi_group_pad, multi_next_group), checked without a GPU: tests/host/multi_group_check.cpp (own main, no HIP) is compiled against the
header with the host compiler behind the Makefile's hipcc, once plainly and once with -fsanitize=address,undefined.  Every hot width of a
mid-width context maps to a group width that has kernel instances, and the groups plus the single left-over column cover any column count."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cglb_amd", "csrc")
HOT_WIDTHS = (48, 64, 80, 96)   # cglb_internal.h: mid_dim


def _hipcc():
    text = open(os.path.join(CSRC, "Makefile")).read()
    return os.environ.get("HIPCC") or re.search(r"^HIPCC \?= (\S+)", text, re.M).group(1)


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def program(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("multi_group") / request.param)
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if request.param == "sanitized" else ["-O2"]
    cmd = [_hipcc(), "-x", "c++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, "-I", CSRC,
           os.path.join(ROOT, "tests", "host", "multi_group_check.cpp"), "-o", exe]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr

    def run(commands):
        out = subprocess.run([exe], input="".join(c + "\n" for c in commands), capture_output=True, text=True)
        assert out.returncode == 0 and not out.stderr, out.stderr
        lines = out.stdout.split("\n")[:-1]
        assert len(lines) == len(commands)
        return [[int(x) for x in line.split()] for line in lines]
    return run


def test_every_hot_width_has_instances(program):
    src = open(os.path.join(CSRC, "kernels_kff_multi_mid.hip")).read()
    for dh, (group, p2, p4, p8) in zip(HOT_WIDTHS, program([f"rule {dh}" for dh in HOT_WIDTHS])):
        assert group in (2, 4, 8), dh
        assert f"MULTI_MID_CASE({dh})" in src                      # the width is dispatched ...
        for sp, part in ((2, p2), (4, p4), (8, p8)):               # ... and every S_pad up to its group width has a batch geometry
            if sp <= group:
                assert part in (8, 16) and part % sp == 0, (dh, sp)
            else:
                assert part == 0, (dh, sp)
    # anything that is no hot width has no instance: the product falls back
    assert program(["rule 32", "rule 40", "rule 97", "rule 128", "rule 0"]) == [[0, 0, 0, 0]] * 5


def test_groups_and_the_left_over_cover_any_column_count(program):
    widths = sorted({program([f"rule {dh}"])[0][0] for dh in HOT_WIDTHS} | {2, 4, 8})
    cases = [(s, g) for g in widths for s in range(1, 18)]
    for (s, g), groups in zip(cases, program([f"groups {s} {g}" for s, g in cases])):
        assert sum(groups) == s, (s, g)
        assert all(1 <= sg <= g for sg in groups), (s, g)
        assert all(sg == g for sg in groups[:-1]), (s, g)          # full groups first
        assert groups.count(1) <= 1 and (1 not in groups[:-1])     # at most one single column, and it is the last: it takes the mat-vec
    assert program(["groups 0 8"]) == [[]]
