"""The two chunk rules of the row-slab products (tests/slab_rules.py, mirroring cglb_amd/csrc/row_slab.h) and the column split of the K_ff gradient
passes (cglb_amd/csrc/grad_pass.h) at hand-derived values.  Every expected pair is (chunks, chunk length); the arithmetic is in the comments."""
import slab_rules as rules


def test_pair_split_forced():
    # 3 chunks of ceil(1000 / 3) = 334 (even already); 3 * 334 >= 1000 > 2 * 334
    assert rules.pair_split(3, 1, 1000, 512, True) == (3, 334)
    # ceil(1000 / 7) = 143, odd -> 144 when even; 6 * 144 = 864 < 1000, so still 7 chunks; 7 * 143 = 1001
    assert rules.pair_split(7, 1, 1000, 512, True) == (7, 144)
    assert rules.pair_split(7, 1, 1000, 512, False) == (7, 143)
    # a forced split beyond ceil(63 / 64) = 1 is cut to 1
    assert rules.pair_split(7, 1, 63, 512, True) == (1, 64)
    assert rules.pair_split(7, 1, 63, 512, False) == (1, 63)


def test_pair_split_capped_by_64_column_chunks():
    # one row block asks for 8192 chunks; ceil(1000 / 64) = 16 allows 16 of ceil(1000 / 16) = 63 -> 64: 16 * 64 = 1024, 15 * 64 = 960
    assert rules.pair_split(0, 1, 1000, 512, True) == (16, 64)
    assert rules.pair_split(0, 1, 1000, 512, False) == (16, 63)   # 16 * 63 = 1008, 15 * 63 = 945
    # 65 columns: 2 chunks of 33 -> 34
    assert rules.pair_split(0, 1, 65, 512, True) == (2, 34)
    assert rules.pair_split(0, 1, 65, 512, False) == (2, 33)
    assert rules.pair_split(0, 1, 1, 512, True) == (1, 2)
    assert rules.pair_split(0, 1, 1, 512, False) == (1, 1)


def test_pair_split_by_row_blocks_and_slot_cap():
    # 40 row blocks: ceil(8192 / 40) = 205 chunks of ceil(100000 / 205) = 488; 204 * 488 = 99552 < 100000 <= 205 * 488
    assert rules.pair_split(0, 40, 100000, 512, True) == (205, 488)
    # the slot cap 256 below both 8192 and ceil(100000 / 64) = 1563: ceil(100000 / 256) = 391 -> 392; 255 * 392 = 99960 < 100000
    assert rules.pair_split(0, 1, 100000, 256, True) == (256, 392)
    assert rules.pair_split(0, 1, 100000, 256, False) == (256, 391)   # 255 * 391 = 99705


def test_slot_cap():
    assert rules.slot_cap(1, 66) == 256                  # the slab is no limit: SLOTS
    # 4096 rows of width 32: 2 columns (or weight slots) x 33 = 66 doubles a row, 2^24 / (4096 * 66) = 62.06
    assert 4096 * 66 * 62 <= 1 << 24 < 4096 * 66 * 63
    assert rules.slot_cap(4096, 2 * 33) == 62
    assert rules.slot_cap(1 << 24, 2) == 1               # never below one chunk
    # ... and the split it gives: 16 row blocks ask for 512, the cap allows 62 chunks of ceil(100000 / 62) = 1613 -> 1614; 61 * 1614 = 98454
    assert rules.pair_split(0, 16, 100000, 62, True) == (62, 1614)
    assert rules.pair_split(0, 16, 100000, 62, False) == (62, 1613)


def test_feature_split():
    assert rules.feature_split(1024, 1, 1) == (1, 1)
    assert rules.feature_split(1024, 1, 63) == (1, 63)   # F < 64: one chunk
    assert rules.feature_split(1024, 1, 65) == (2, 33)
    # one row block asks for 2048, SLOTS allows 256 (ceil(16385 / 64) = 257): chunks of ceil(16385 / 256) = 65, of which ceil(16385 / 65) = 253
    assert rules.feature_split(1024, 1024, 16385) == (253, 65)
    assert rules.feature_split(1024, 1025, 16385) == (253, 65)   # two row blocks ask for 1024: the same
    # 16 row blocks ask for 128; ceil(1000 / 64) = 16 chunks of ceil(1000 / 16) = 63 (no even rounding in this rule)
    assert rules.feature_split(256, 4096, 1000) == (16, 63)
    # ... capped by a slot cap of 62: chunks of ceil(100000 / 62) = 1613
    assert rules.feature_split(256, 4096, 100000, 62) == (62, 1613)


# ---- grad_pass_split: the five formulas the gradient launchers carried before the rule had one place, transcribed once ----
def _old_narrow_range(bx, ncols, sym):
    """launch_grad_kff, per column range (the square block with sym, the off-diagonal ranges without)"""
    js = (8192 + bx - 1) // bx
    if sym:
        js *= 2
    if js > 1024:
        js = 1024
    if js > (ncols + 63) // 64:
        js = (ncols + 63) // 64
    if js < 1:
        js = 1
    jchunk = (ncols + js - 1) // js
    return (ncols + jchunk - 1) // jchunk, jchunk


def _old_symmetric(bx, n):
    """launch_grad_kff_cyclic, launch_grad_kff_mid, grad_multi_group and grad_multi_mid_generic: the same text four times"""
    js = 2 * ((8192 + bx - 1) // bx)
    if js > 1024:
        js = 1024
    if js > (n + 63) // 64:
        js = (n + 63) // 64
    if js < 1:
        js = 1
    jchunk = (n + js - 1) // js
    return (n + jchunk - 1) // jchunk, jchunk


_GRAD_BX = list(range(1, 401))
_GRAD_NCOLS = sorted(set(list(range(1, 260)) + [4095, 4096, 4097, 8191, 8192, 8193, 65535, 65536, 65537, 131071, 131072, 131073, 199999, 200000]
                         + [1 + 997 * k for k in range(201)] + [64 * k + r for k in (15, 16, 1023, 1024, 1025, 2047) for r in (-1, 0, 1)]))


def test_grad_pass_split_is_the_old_formulas():
    assert _GRAD_NCOLS[0] == 1 and _GRAD_NCOLS[-1] == 200000
    for bx in _GRAD_BX:
        for ncols in _GRAD_NCOLS:
            assert rules.grad_pass_split(bx, ncols, False) == _old_narrow_range(bx, ncols, False), (bx, ncols)
            assert rules.grad_pass_split(bx, ncols, True) == _old_narrow_range(bx, ncols, True) == _old_symmetric(bx, ncols), (bx, ncols)


def test_grad_pass_split_caps():
    # js hits 1024: one row block asks for 8192 (16384 symmetric); ceil(200000 / 64) = 3125 allows it; chunks of ceil(200000 / 1024) = 196, of which
    # ceil(200000 / 196) = 1021 (1020 * 196 = 199920 < 200000 <= 1021 * 196)
    assert rules.grad_pass_split(1, 200000, False) == (1021, 196)
    assert rules.grad_pass_split(1, 200000, True) == (1021, 196)
    # ... and just below the cap: 9 row blocks ask for ceil(8192 / 9) = 911 chunks of ceil(200000 / 911) = 220, of which ceil(200000 / 220) = 910;
    # symmetric 1822 -> 1024
    assert rules.grad_pass_split(9, 200000, False) == (910, 220)
    assert rules.grad_pass_split(9, 200000, True) == (1021, 196)
    # js hits ceil(ncols / 64): 1000 columns allow 16 chunks of ceil(1000 / 16) = 63; 16 * 63 = 1008, 15 * 63 = 945
    assert rules.grad_pass_split(1, 1000, False) == (16, 63)
    assert rules.grad_pass_split(1, 1000, True) == (16, 63)
    assert rules.grad_pass_split(1, 65, True) == (2, 33)
    # ncols < 64: one chunk, whatever the row blocks ask for
    assert rules.grad_pass_split(1, 63, True) == (1, 63)
    assert rules.grad_pass_split(1, 1, False) == (1, 1)
    assert rules.grad_pass_split(400, 2, True) == (1, 2)
    # bx > 8192: ceil(8192 / 10000) = 1 chunk, 2 for the symmetric form: ceil(100000 / 2) = 50000
    assert rules.grad_pass_split(10000, 100000, False) == (1, 100000)
    assert rules.grad_pass_split(10000, 100000, True) == (2, 50000)
    # the doubling is not ceil(16384 / bx): 19 row blocks ask for 2 * ceil(8192 / 19) = 2 * 432 = 864 chunks, not ceil(16384 / 19) = 863.  At
    # 55296 = 864 * 64 columns that is 864 chunks of 64 against ceil(55296 / 863) = 65 -> ceil(55296 / 65) = 851 chunks
    assert rules.grad_pass_split(19, 55296, True) == (864, 64)
    assert rules.pair_split(0, 19, 55296, 1024, False) == (432, 128)      # the row-slab rule at the same row blocks: no doubling
    assert rules.pair_split(16384 // 19 + 1, 1, 55296, 1024, False) == (851, 65)   # what ceil(16384 / 19) = 863 chunks would give


def test_dealt_blocks():
    # 10 row blocks over 3 ranks: 0, 3, 6, 9 | 1, 4, 7 | 2, 5, 8
    assert [rules.dealt_blocks(10, 3, r) for r in range(3)] == [4, 3, 3]
    # more ranks than blocks: the ranks beyond have none
    assert [rules.dealt_blocks(2, 4, r) for r in range(4)] == [1, 1, 0, 0]
    assert rules.dealt_blocks(7, 1, 0) == 7
    for nb in range(1, 40):
        for world in range(1, 9):
            assert [rules.dealt_blocks(nb, world, r) for r in range(world)] == [len(range(r, nb, world)) for r in range(world)]
