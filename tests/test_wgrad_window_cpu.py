"""A model of wgrad_h2_kernel's input window (csrc/wgrad_mfma.hip), old and new address maps side by side, without a GPU.

Old: 128 slots of 128 bytes per plane, circular (`& 127` per lane), 16-byte-granular XOR swizzle by the absolute slot.
New: 128 + 16 slots at a fixed pitch, no swizzle; slots 128..143 mirror slots 0..15 (`put` writes a row twice when its slot is
below 16), so a 16-row fragment group that starts at any slot 0..127 never wraps and its address is one per-lane base plus a
wave-uniform `slot * pitch`.

The model stages what the kernel stages (the first tile's re-stage of the 2 x halo older rows, then 32 new rows per tile), and
for every read of the tap loop asks both maps which (tensor row, channel group, plane) the lane gets.  The bank rules are those
of the LDS: an 8-byte transposing read is served per 32-lane half over 64 banks of 4 bytes, an 8-byte store per 16 contiguous
lanes over 32 banks."""
import numpy as np
import pytest

WIN, GUARD, PITCH, TK, RPP = 128, 16, 160, 32, 16
OLD_PLANE, NEW_PLANE = WIN * 128, (WIN + GUARD) * PITCH
LANES = np.arange(64)
LROW = 4 * (LANES >> 4) + ((LANES & 15) >> 2)
COLB = (LANES & 3) * 8


def swz(slot):
    return (slot & 6) << 4


def code(row, c4, plane):
    return ((row + 4096) * 16 + c4) * 2 + plane


def put_old(mem, row, c4, plane):
    slot = row & (WIN - 1)
    mem[(slot * 128 + ((c4 * 8) ^ swz(slot)) + plane * OLD_PLANE) // 8] = code(row, c4, plane)


def put_new(mem, row, c4, plane, pitch=PITCH):
    slot = row & (WIN - 1)
    a = slot * pitch + c4 * 8 + plane * (WIN + GUARD) * pitch
    mem[a // 8] = code(row, c4, plane)
    dup = slot < GUARD
    mem[(a[dup] + WIN * pitch) // 8] = code(row, c4, plane)[dup]


def read_old(q0, sh, half, mtw, mt, plane):
    s0 = q0 + LROW + WIN
    slot_lo = (s0 + sh) & (WIN - 1)
    slot_hi = (slot_lo + 16) & (WIN - 1)
    cs = ((mtw * 64 + COLB) ^ swz(slot_lo)) ^ (mt * 32)
    return ((slot_hi if half else slot_lo) << 7 | cs) + plane * OLD_PLANE


def read_new(q0, sh, half, mtw, mt, plane, pitch=PITCH):
    lane_base = LROW * pitch + mtw * 64 + COLB                   # per lane, tile-invariant
    s = (q0 + 16 * half + sh) & (WIN - 1)                        # wave-uniform
    return lane_base + s * pitch + plane * (WIN + GUARD) * pitch + mt * 32   # (plane, mt: the immediate offset)


@pytest.mark.parametrize("W", range(1, 47))
def test_both_maps_name_the_same_row_channel_and_plane(W):
    """Every W the kernel accepts, 40 tiles of one workgroup (ten wraps of the window), nine taps, both 16-row groups, 64 lanes,
    both waves' channel halves, both m-tiles, both planes: the two maps return the element the MFMA expects, and nothing a
    read touches -- guard slots included -- is unwritten or left over from 128 rows earlier."""
    Wp = W + 1
    halo = Wp + 1
    assert TK + 2 * halo <= WIN
    old = np.full(2 * OLD_PLANE // 8, -1, dtype=np.int64)
    new = np.full(2 * NEW_PLANE // 8, -1, dtype=np.int64)
    c4 = np.tile(np.arange(16), RPP)
    prow = np.repeat(np.arange(RPP), 16)
    for tile in range(40):
        q0 = tile * TK
        staged = [q0 + halo + prow + RPP * u for u in range(2)]
        if tile == 0:   # the first tile chooses the exponent: the 2 x halo older rows are (re-)staged
            staged += [q0 - halo + prow + RPP * u for u in range((2 * 47 + RPP - 1) // RPP)]
            staged = [r[r - (q0 - halo) < 2 * halo] if i >= 2 else r for i, r in enumerate(staged)]
        for rows in staged:
            cc = c4[:rows.size]
            for plane in range(2):
                put_old(old, rows, cc, plane)
                put_new(new, rows, cc, plane)
        for tap in range(9):
            sh = (tap // 3 - 1) * Wp + (tap % 3 - 1)
            for half in range(2):
                for mtw in range(2):
                    for mt in range(2):
                        for plane in range(2):
                            want = code(q0 + 16 * half + sh + LROW, (mtw * 64 + mt * 32 + COLB) // 8, plane)
                            a_new = read_new(q0, sh, half, mtw, mt, plane)
                            assert a_new.max() + 8 <= 2 * NEW_PLANE
                            got_old = old[read_old(q0, sh, half, mtw, mt, plane) // 8]
                            got_new = new[a_new // 8]
                            assert (got_old == want).all() and (got_new == want).all(), (W, tile, tap, half, mtw, mt, plane)


def read_conflicts(addr):
    """Extra LDS cycles of one 8-byte transposing read: per 32-lane half, (distinct addresses on the busiest bank) - 1."""
    extra = 0
    for half in (addr[:32], addr[32:]):
        banks = {}
        for a in np.unique(half):
            for d in (0, 4):
                banks.setdefault(((a + d) // 4) % 64, set()).add(a)
        extra += max(len(v) for v in banks.values()) - 1
    return extra


def store_conflicts(addr):
    """Extra LDS cycles of one 8-byte store: per 16 contiguous lanes, 32 banks."""
    extra = 0
    for g in range(4):
        banks = {}
        for a in np.unique(addr[16 * g:16 * g + 16]):
            for d in (0, 4):
                banks.setdefault(((a + d) // 4) % 32, set()).add(a)
        extra += max(len(v) for v in banks.values()) - 1
    return extra


def pitch_conflicts(pitch):
    """(read, store) conflict cycles summed over every start slot / every row alignment of the window."""
    rd = st = 0
    for s in range(WIN):
        for mtw in range(2):
            for mt in range(2):
                rd += read_conflicts(read_new(s, 0, 0, mtw, mt, 0, pitch))
    tid = np.arange(64)
    for row0 in range(WIN):           # a wave stores four consecutive rows, 16 lanes x 8 bytes each
        slot = (row0 + tid // 16) & (WIN - 1)
        st += store_conflicts(slot * pitch + (tid % 16) * 8)
        st += store_conflicts(slot * pitch + (tid % 16) * 8 + WIN * pitch)   # the guard copy
    return rd, st


def test_the_pitch_is_the_smallest_without_bank_conflicts():
    """Brute force over pitches 128 + 8 k and every row alignment: 160 is the first at which neither the transposing reads nor
    the 8-byte stores conflict (136, 144 and 152 put two of a half-wave's eight rows on the same banks; 128 all eight)."""
    table = {p: pitch_conflicts(p) for p in range(128, 200, 8)}
    assert table[PITCH] == (0, 0)
    assert min(p for p, c in table.items() if c == (0, 0)) == PITCH
    assert table[128][0] > 0 and table[144][0] > 0
    assert all(c[1] == 0 for c in table.values())     # a store's 16 lanes cover one row's 128 bytes: any pitch will do
    # the old map bought the same freedom with its swizzle
    for q0 in range(0, WIN, 1):
        assert read_conflicts(read_old(q0, 0, 0, 0, 0, 0)) == 0


def test_the_window_fits_two_workgroups_per_cu():
    """launch_wgrad_h2's dynamic LDS with the BatchNorm backward inside (the largest form): at most 80 KiB."""
    window = 2 * (WIN + GUARD) * PITCH
    lds = window + 2 * TK * 128 + RPP * 64 * 4 + 12 * 4 + (2 + 11) * 64 * 4 + 256 + 2 * 8192 + 4 * 256
    assert window == 46080 and lds == 79408 and lds <= 80 * 1024
    assert (2 * NEW_PLANE) % 256 == 0                   # the dout tile behind it keeps its 128-byte alignment (XOR-ed addresses)
    assert NEW_PLANE + 32 < 65536                       # plane + m-tile fit the 16-bit immediate offset
