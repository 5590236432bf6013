"""The yardstick of tests/test_score_cpu.py and tests/test_score_gpu.py: a per-millisecond model of the reference's evaluation
(analysis/preprocess.py, analysis/analyse.py, analysis/utils.py), transcribed loop by loop.  A set of milliseconds is a boolean
array (element m is millisecond m), (lo, hi] is the slice lo + 1 .. hi, union / difference / intersection are | & ~, a length is a
count of True -- what utils.p_len does by iterating the interval.  Nothing here is shared with the product (sweep_eval.py,
csrc/score.hip).  Also the seeded transcript tables the tests feed both with."""
import csv
import os

import numpy as np

FACTOR = 1000 / 1                       # config.py: frame_duration = 1 ms


def to_frames(t):
    return round(t * FACTOR)            # Python's round: half to even


def to_sec(n):
    return n / FACTOR


class Model:
    """N: the universe (milliseconds 0 .. N - 1); every interval end of rows, channels and predictions must be below it."""

    def __init__(self, rows, chans, N):
        self.N = N
        self.chan_to_part = {}
        for c in chans:
            if c["part_id"] not in (None, ""):
                self.chan_to_part.setdefault(c["meeting_id"], {})[c["chan"]] = c["part_id"]
        self.invalid = self._index_from([r for r in rows if r["type"] == "invalid"])
        self.laugh = self._laugh_index([r for r in rows if r["type"] == "laugh"], self.invalid)
        self.speech = self._index_from([r for r in rows if r["type"] == "speech"])
        self.noise = self._index_from([r for r in rows if r["type"] == "noise"])
        self.silence = {}
        for c in chans:                                                    # create_silence_index
            if c["part_id"] in (None, ""):
                continue
            m, p = c["meeting_id"], c["part_id"]
            seg = self.oc(0, to_frames(c["length"]))
            for idx in (self.laugh, self.invalid, self.speech, self.noise):
                seg = seg & ~self.get(idx, m, p)
            self.silence.setdefault(m, {})[p] = seg
        self.laugh_rows = {}
        for r in rows:
            if r["type"] == "laugh":
                self.laugh_rows[r["meeting_id"]] = self.laugh_rows.get(r["meeting_id"], 0) + 1

    def oc(self, lo, hi):
        s = np.zeros(self.N, bool)
        assert hi < self.N and lo >= 0
        if hi > lo:
            s[lo + 1:hi + 1] = True
        return s

    def get(self, index, m, p):
        return index.get(m, {}).get(p, np.zeros(self.N, bool))

    def _append(self, index, row):
        m, p = row["meeting_id"], row["part_id"]
        index.setdefault(m, {"tot_len": 0, "tot_events": 0})
        seg = self.oc(to_frames(row["start"]), to_frames(row["end"]))
        index[m][p] = index[m][p] | seg if p in index[m] else seg
        index[m]["tot_len"] += to_sec(int(seg.sum()))
        index[m]["tot_events"] += 1

    @staticmethod
    def _grouped(rows):
        """meetings ascending, rows by start, participants ascending (the groupby / sort_values / groupby of preprocess.py)"""
        for m in sorted({r["meeting_id"] for r in rows}):
            mrows = sorted([r for r in rows if r["meeting_id"] == m], key=lambda r: r["start"])
            for p in sorted({r["part_id"] for r in mrows}):
                for r in mrows:
                    if r["part_id"] == p:
                        yield r

    def _index_from(self, rows):
        index = {}
        for r in self._grouped(rows):
            self._append(index, r)
        return index

    def _laugh_index(self, rows, invalid_index):
        index = {}
        for r in self._grouped(rows):
            index.setdefault(r["meeting_id"], {"tot_len": 0, "tot_events": 0})
            if r["length"] < 0.2 or r["laugh_type"] == "breath-laugh":    # seg_invalid
                self._append(invalid_index, r)
                continue
            self._append(index, r)
        return index

    def tot(self, index, m, what):
        return index.get(m, {}).get(what, 0)

    # ---- analyse.py ---------------------------------------------------------------------------------------------------------------
    def score(self, spans, m, chan):
        """The seven integers of one channel and one setting: eval_preds' loop over the rows of one participant + laugh_match, in
        milliseconds.  spans: [(start_s, end_s)]."""
        p = self.chan_to_part.get(m, {}).get(chan)
        inv = self.get(self.invalid, m, p)
        n_pred = n_valid = 0
        union = np.zeros(self.N, bool)
        for start, end in spans:
            a, b = to_frames(start), to_frames(end)
            pred = self.oc(a, b)
            n_pred += 1
            contained = not (pred & ~inv).any()                            # (an empty prediction is contained)
            if not inv.any() or not contained:
                n_valid += 1
            union = union | pred
        union = union & ~inv
        out = [n_pred, n_valid, int(union.sum())]
        for idx in (self.laugh, self.speech, self.noise):
            out.append(int((union & self.get(idx, m, p)).sum()))
        out.append(int((union & self.silence.get(m, {}).get(p, np.zeros(self.N, bool))).sum()))
        return tuple(out)

    def eval_preds(self, per_part_scores, m, thr, min_l):
        """eval_preds :152-225 from the per-participant integers: per_part_scores {part_id: 7 ints}."""
        corr_t = incorr_t = speech_t = noise_t = silence_t = 0
        n_pred = n_valid = 0
        for p in sorted(per_part_scores):
            s = per_part_scores[p]
            n_pred += s[0]
            n_valid += s[1]
            if s[0] == 0:
                continue
            pred_length = to_sec(s[2])
            correct = to_sec(s[3])
            incorrect = pred_length - correct
            corr_t += correct
            incorr_t += incorrect
            speech_t += to_sec(s[4])
            noise_t += to_sec(s[5])
            silence_t += to_sec(s[6])
        tot_pred = corr_t + incorr_t
        prec = 1 if tot_pred == 0 else corr_t / tot_pred
        tot_transc = self.tot(self.laugh, m, "tot_len")
        recall = float("NaN") if tot_transc == 0 else corr_t / tot_transc
        return [m, thr, min_l, prec, recall, corr_t, tot_pred, tot_transc, n_pred, n_valid, self.laugh_rows.get(m, 0), speech_t,
                noise_t, silence_t]


def make_rows(seed, meeting, parts, duration_s, n_per_type=40, max_len_s=3.0):
    """Seeded transcript rows for the participants of one meeting: overlapping and adjacent rows, zero-length rows, half-way
    millisecond values, breath-laughs and short laughs."""
    rng = np.random.default_rng(seed)
    rows = []
    for p in parts:
        for kind in ("laugh", "speech", "noise", "invalid"):
            starts = np.sort(rng.random(n_per_type)) * duration_s
            for i, s in enumerate(starts):
                s = round(float(s), 3) + (0.0005 if i % 7 == 0 else 0.0)          # x.xxx5: a half-way value
                length = round(float(rng.random() * max_len_s), 3)
                if i % 11 == 0:
                    length = 0.0                                                   # start == end
                if i % 5 == 0 and kind == "laugh":
                    length = round(float(rng.random() * 0.19), 3)                  # shorter than 0.2 s: invalid
                e = s + length
                if i % 13 == 0 and i + 1 < len(starts):
                    e = round(float(starts[i + 1]), 3)                             # adjacent to (or overlapping) the next row
                    if (i + 1) % 7 == 0:
                        e += 0.0005
                    e = max(e, s)
                lt = ("breath-laugh" if i % 6 == 0 else "laugh") if kind == "laugh" else None
                rows.append({"meeting_id": meeting, "part_id": p, "chan": None, "start": s, "end": e, "length": e - s, "type": kind,
                             "laugh_type": lt})
    order = rng.permutation(len(rows))
    return [rows[i] for i in order]


def write_corpus(tmp_path, T=3000):
    """Three synthetic channels of two meetings as evaluate_sweep.py reads them; returns its arguments."""
    rows = make_rows(11, "Bmr001", ["fe001", "me002"], 30.0, n_per_type=15) + make_rows(12, "Bed002", ["mn003"], 30.0, n_per_type=15)
    chans = [{"meeting_id": "Bmr001", "part_id": "fe001", "chan": "chan0", "length": 30.0},
             {"meeting_id": "Bmr001", "part_id": "me002", "chan": "chan3", "length": 29.317},
             {"meeting_id": "Bmr001", "part_id": "", "chan": "chan5", "length": 30.0},
             {"meeting_id": "Bed002", "part_id": "mn003", "chan": "chan1", "length": 25.0049375}]
    part_chan = {(c["meeting_id"], c["part_id"]): c["chan"] for c in chans}
    with open(tmp_path / "transcripts.csv", "w", newline="") as f:
        w = csv.DictWriter(f, fieldnames=["meeting_id", "part_id", "chan", "start", "end", "length", "type", "laugh_type"])
        w.writeheader()
        for r in rows:
            w.writerow(dict(r, chan=part_chan[(r["meeting_id"], r["part_id"])], laugh_type=r["laugh_type"] or ""))
    with open(tmp_path / "channels.csv", "w", newline="") as f:
        w = csv.DictWriter(f, fieldnames=["meeting_id", "part_id", "chan", "length"])
        w.writeheader()
        w.writerows(chans)
    for i, (m, chan, n) in enumerate((("Bmr001", "chan0", T), ("Bmr001", "chan3", T - 70), ("Bed002", "chan1", T - 500))):
        os.makedirs(tmp_path / "probs" / m, exist_ok=True)
        np.save(tmp_path / "probs" / m / f"{chan}.npy", _track(30 + i, n).astype(np.float32))
    return ["--probs_dir", str(tmp_path / "probs"), "--transcripts", str(tmp_path / "transcripts.csv"), "--channels",
            str(tmp_path / "channels.csv"), "--thresholds", "0.2,0.5,0.8", "--min_lengths", "0.0,0.2"]


def _track(seed, n):
    from oracle import recipe
    return recipe.make_prob_track(seed, n)
