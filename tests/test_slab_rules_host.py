"""The two chunk rules of the row-slab products (tests/slab_rules.py, mirroring cglb_amd/csrc/row_slab.h) at hand-derived values.  Every expected
pair is (chunks, chunk length); the arithmetic is in the comments."""
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
