"""The two chunk rules of the row-slab products (cglb_amd/csrc/row_slab.h) and the column split of the K_ff gradient passes
(cglb_amd/csrc/grad_pass.h), once (test helper, not a test module).  All return (chunks, chunk length).  The *_ref modules apply the
row-slab rules at their kernel's rows per block and slot cap."""
from __future__ import annotations

SLOTS, SLAB = 256, 1 << 24          # ROW_SLAB_SLOTS, ROW_SLAB_GRAD_DOUBLES
MIN_CHUNK, TARGET_WG = 64, 2048     # FEATURE_MIN_CHUNK, FEATURE_TARGET_WG


def _cdiv(a: int, b: int) -> int:
    return (a + b - 1) // b


def pair_split(forced: int, row_blocks: int, n_cols: int, slot_cap: int, even: bool):
    """row_slab_pair_split: `forced` (kff_jsplit) or ceil(8192 / row blocks) chunks, within 1 .. min(slot_cap, ceil(n_cols / 64))."""
    js = forced if forced > 0 else _cdiv(8192, row_blocks)
    js = max(1, min(js, slot_cap, _cdiv(n_cols, 64)))
    chunk = _cdiv(n_cols, js)
    if even:
        chunk = (chunk + 1) & ~1
    return _cdiv(n_cols, chunk), chunk


def feature_split(rows_per_block: int, n_rows: int, F: int, slot_cap: int = SLOTS):
    """row_slab_feature_split: ceil(TARGET_WG / row blocks) chunks, within 1 .. min(slot_cap, ceil(F / MIN_CHUNK))."""
    bx = max(_cdiv(n_rows, rows_per_block), 1)   # the library needs n_rows >= 1 (no rows: no launch); the tolerance helpers may ask at 0
    js = max(1, min(_cdiv(TARGET_WG, bx), slot_cap, _cdiv(F, MIN_CHUNK)))
    chunk = _cdiv(F, js)
    return _cdiv(F, chunk), chunk


def slot_cap(n_rows: int, row_doubles: int) -> int:
    """row_slab_slot_cap: most chunks of a gradient launch whose rows keep row_doubles partial sums each."""
    return max(1, min(SLOTS, SLAB // (n_rows * row_doubles)))


GRAD_TARGET_WG, GRAD_MAX_CHUNKS = 8192, 1024   # GRAD_PASS_TARGET_WG, the cap of grad_pass_split


def grad_pass_split(row_blocks: int, n_cols: int, sym: bool):
    """grad_pass_split: ceil(8192 / row blocks) chunks, twice that for the symmetric form, within 1 .. min(1024, ceil(n_cols / 64))."""
    js = _cdiv(GRAD_TARGET_WG, row_blocks) * (2 if sym else 1)
    js = max(1, min(js, GRAD_MAX_CHUNKS, _cdiv(n_cols, 64)))
    chunk = _cdiv(n_cols, js)
    return _cdiv(n_cols, chunk), chunk


def dealt_blocks(nb: int, world: int, rank: int) -> int:
    """grad_pass_dealt_blocks: row blocks rank, rank + world, ... below nb."""
    return (nb - rank + world - 1) // world if rank < nb else 0
