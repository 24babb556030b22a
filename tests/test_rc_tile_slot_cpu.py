"""Slot function of the recompute product's wave-private LDS tile
(csrc/megba/gpu/rc_tile.hpp) through the _core.rc_tile_slot binding: 64 rows
of four 16-byte chunks in 4 KiB.  It must be a bijection, and neither the
128-bit stores that fill the tile nor the 128-bit loads that read a lane's own
row may put two lanes of one LDS lane group on one bank.

Lane groups and bank rules are those of the CDNA4 LDS: a ds_read_b128 is
served in four groups of 16 lanes over 64 four-byte banks, a ds_write_b128 in
eight groups of 8 consecutive lanes over 32 banks.
"""
from megba_amd import _core

ROWS, CHUNKS, CHUNK_BYTES = 64, 4, 16

READ_GROUPS = [
    [*range(0, 4), *range(12, 16), *range(20, 28)],
    [*range(4, 12), *range(16, 20), *range(28, 32)],
    [*range(32, 36), *range(44, 48), *range(52, 60)],
    [*range(36, 44), *range(48, 52), *range(60, 64)],
]
WRITE_GROUPS = [list(range(8 * g, 8 * g + 8)) for g in range(8)]


def _banks(offset, nbanks):
    return {(offset // 4 + d) % nbanks for d in range(CHUNK_BYTES // 4)}


def _assert_conflict_free(groups, offsets, nbanks):
    for grp in groups:
        seen = set()
        for lane in grp:
            b = _banks(offsets[lane], nbanks)
            assert not (b & seen), (grp, lane)
            seen |= b


def test_groups_cover_the_wave():
    for groups in (READ_GROUPS, WRITE_GROUPS):
        assert sorted(l for g in groups for l in g) == list(range(64))


def test_slot_is_a_bijection_on_the_tile():
    assert _core.rc_tile_bytes == ROWS * CHUNKS * CHUNK_BYTES
    offs = [_core.rc_tile_slot(r, c) for r in range(ROWS) for c in range(CHUNKS)]
    assert sorted(offs) == list(range(0, _core.rc_tile_bytes, CHUNK_BYTES))
    # a row stays inside its own 64 bytes
    for r in range(ROWS):
        assert {_core.rc_tile_slot(r, c) // 64 for c in range(CHUNKS)} == {r}


def test_reads_are_conflict_free():
    """Read k of a round: lane L reads chunk k of its own row L."""
    for k in range(CHUNKS):
        offs = [_core.rc_tile_slot(lane, k) for lane in range(64)]
        _assert_conflict_free(READ_GROUPS, offs, 64)


def test_writes_are_conflict_free():
    """Store i of a round: lane L writes chunk L % 4 of row 16 i + L // 4."""
    for i in range(4):
        offs = [_core.rc_tile_slot(16 * i + lane // 4, lane % 4)
                for lane in range(64)]
        _assert_conflict_free(WRITE_GROUPS, offs, 32)


def test_unswizzled_layout_would_conflict():
    """The check has teeth: rows at a plain 64-byte pitch conflict on reads."""
    offs = [lane * 64 for lane in range(64)]
    try:
        _assert_conflict_free(READ_GROUPS, offs, 64)
    except AssertionError:
        return
    raise AssertionError("plain layout passed the bank check")


def test_staged_lds_bytes():
    """Accumulators rounded up to 16 bytes, then one 4 KiB tile per wave."""
    f = _core.rc_staged_lds_bytes
    # Venice-1778 fp64 at 512 threads: 128 016 + 32 768
    assert f(1778 * 9, 8, 8) == 160784
    # accumulators that end off a 16-byte boundary: 1656 -> 1664, 828 -> 832
    assert f(23 * 9, 8, 8) == 1664 + 8 * 4096
    assert f(23 * 9, 4, 3) == 832 + 3 * 4096
    assert f(24 * 9, 8, 1) == 1728 + 4096
    for nc in range(9, 9 * 40, 9):
        for eb in (4, 8):
            off = f(nc, eb, 0)
            assert off % 16 == 0 and 0 <= off - nc * eb < 16
