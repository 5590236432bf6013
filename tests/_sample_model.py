"""Second implementation of the segment-sampling convention, in Python integers: written from the text next to
`lad_sample_segments` in include/lad_hip.h, not from the kernel or from sampling.py.  Philox and mulhi are those of
tests/_augment_model.py (pinned there to Random123's known answers); the transcript rows come from tests/_score_model.py, whose
per-millisecond boolean sets are the brute-force side of the frame rule."""
import numpy as np

from _augment_model import mulhi, philox4x32_10

FIXED, POOL_ROW, POOL_MEASURE = 0, 1, 2
TAG = 0x53414D50
M32 = 0xFFFFFFFF


def words(seed, epoch, row_id):
    row_id, seed = int(row_id) & (2 ** 64 - 1), int(seed)
    return philox4x32_10((row_id & M32, row_id >> 32, int(epoch), TAG), (seed & M32, seed >> 32))


def pool_cum_of(regions, pool_off, T):
    """(pool_cum per region, total per pool): windows of T frames inside the regions before j in j's pool."""
    regions = np.asarray(regions, np.int64).reshape(-1, 3)
    cum = np.zeros(len(regions), np.int64)
    total = np.zeros(len(pool_off) - 1, np.int64)
    for p in range(len(pool_off) - 1):
        acc = 0
        for j in range(int(pool_off[p]), int(pool_off[p + 1])):
            cum[j] = acc
            acc += max(int(regions[j, 2]) - int(regions[j, 1]) - T + 1, 0)
        total[p] = acc
    return cum, total


def draw_row(kind, src, regions, pool_off, pool_cum, T, r):
    """One row: (chan, first, count, region index, u) -- u the measure draw of a POOL_MEASURE row, else None."""
    u = None
    if kind == FIXED:
        j = int(src)
    else:
        o0, o1 = int(pool_off[src]), int(pool_off[src + 1])
        assert o1 > o0
        if kind == POOL_ROW:
            j = o0 + mulhi(r[0], o1 - o0)
        else:
            chan, lo, hi = (int(v) for v in regions[o1 - 1])
            M = int(pool_cum[o1 - 1]) + (hi - lo - T + 1)
            assert 1 <= M < 2 ** 32
            u = mulhi(r[0], M)
            j = max(k for k in range(o0, o1) if int(pool_cum[k]) <= u)
    chan, lo, hi = (int(v) for v in regions[j])
    if kind == POOL_MEASURE:
        assert hi - lo >= T
        return chan, lo + (u - int(pool_cum[j])), T, j, u
    n = min(T, hi - lo)
    return chan, lo + mulhi(r[1], hi - lo - n + 1), n, j, u


def draw(kind, src, regions, pool_off, pool_cum, T, seed, epoch, row_id=None, detail=False):
    """The whole table: chan int32, first int64, count int32 (and region, u lists with detail=True)."""
    n = len(kind)
    chan, first, count, reg, us = np.zeros(n, np.int32), np.zeros(n, np.int64), np.zeros(n, np.int32), np.zeros(n, np.int32), []
    for i in range(n):
        rid = i if row_id is None else int(row_id[i])
        chan[i], first[i], count[i], reg[i], u = draw_row(int(kind[i]), int(src[i]), regions, pool_off, pool_cum, T, words(seed, epoch, rid))
        us.append(u)
    return (chan, first, count, reg, us) if detail else (chan, first, count)


# ---- frames and milliseconds -----------------------------------------------------------------------------------------------------
def frame_inside(member, f, fps):
    """Frame f spans (1000 f / fps, 1000 (f + 1) / fps]; it lies inside the set iff every millisecond cell (m - 1, m] it meets does:
    m from floor(1000 f / fps) + 1 to ceil(1000 (f + 1) / fps).  member[m]: millisecond m = the cell (m - 1, m] is in the set."""
    lo, hi = 1000 * f // fps, -((-1000 * (f + 1)) // fps)
    return hi < len(member) and bool(member[lo + 1:hi + 1].all())


def frames_inside(member, fps, frames_c):
    """bool per frame of the channel."""
    return np.asarray([frame_inside(member, f, fps) for f in range(frames_c)], bool)


def runs(mask):
    """[(a, b)] of the maximal runs of True."""
    m = np.concatenate([[False], np.asarray(mask, bool), [False]])
    d = np.flatnonzero(m[1:] != m[:-1])
    return [(int(a), int(b)) for a, b in zip(d[0::2], d[1::2])]


def hull(first, count, fps):
    return 1000 * int(first) // fps, -((-1000 * (int(first) + int(count))) // fps)


def coverage_ms(member, first, count, fps):
    """Milliseconds of the set inside the hull of the window."""
    lo, hi = hull(max(int(first), 0), max(int(count), 0), fps)
    return int(np.asarray(member[lo + 1:hi + 1]).sum())


def member_of(intervals, N):
    """Boolean millisecond set of (lo, hi] rows."""
    m = np.zeros(N, bool)
    for lo, hi in intervals:
        m[int(lo) + 1:int(hi) + 1] = True
    return m


# ---- the corpus of the sampler tests ---------------------------------------------------------------------------------------------
def corpus(n_per_type=12, duration=60.0, max_len_s=2.0):
    """2 meetings x 3 participants: (rows, channels)."""
    from _score_model import make_rows
    meetings = {"Bmr001": ["fe001", "me002", "me003"], "Bed002": ["mn004", "fe005", "me006"]}
    rows, chans = [], []
    for k, (m, parts) in enumerate(meetings.items()):
        rows += make_rows(21 + k, m, parts, duration, n_per_type=n_per_type, max_len_s=max_len_s)
        for i, p in enumerate(parts):
            chans.append({"meeting_id": m, "part_id": p, "chan": f"chan{2 * i + k}", "length": duration - 0.317 * i})
    part_chan = {(c["meeting_id"], c["part_id"]): c["chan"] for c in chans}
    rows = [dict(r, chan=part_chan[(r["meeting_id"], r["part_id"])]) for r in rows]
    return rows, chans
