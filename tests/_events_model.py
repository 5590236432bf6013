"""The yardstick of tests/test_events_cpu.py and tests/test_events_gpu.py: the convention above lad_score_events in
include/lad_hip.h, restated on the per-millisecond sets of tests/_score_model.py.  A set of milliseconds is a boolean array, an event
is a maximal run of True in LAUGH & ~INVALID, a prediction is the slice a + 1 .. b, and every (event, prediction) pair is looked
at on its own: its overlap is a count of True.  Slow by design; the tests give it a subset of settings.  Nothing here is shared with
the product (sweep_eval.py, csrc/events.hip)."""
import numpy as np

import _score_model as sm


class EventModel:
    def __init__(self, rows, chans, N):
        self.sets = sm.Model(rows, chans, N)
        self.N = N

    def laugh_and_invalid(self, m, chan):
        p = self.sets.chan_to_part.get(m, {}).get(chan)
        inv = self.sets.get(self.sets.invalid, m, p)
        return self.sets.get(self.sets.laugh, m, p) & ~inv, inv

    def events(self, m, chan):
        """[(lo, hi)]: the maximal intervals (lo, hi] of LAUGH minus INVALID, ascending."""
        laugh, _ = self.laugh_and_invalid(m, chan)
        out, lo = [], None
        for ms in range(self.N):
            if laugh[ms] and lo is None:
                lo = ms - 1
            if not laugh[ms] and lo is not None:
                out.append((lo, ms - 1))
                lo = None
        assert lo is None                                                  # (the universe ends behind every interval)
        return out

    def pairs(self, spans, m, chan, events=None):
        """What does not depend on the criteria: per prediction (|pred n LAUGH|, |pred \\ INVALID|), per event [(overlap, a, b)] of
        its links in table order.  spans: [(start_s, end_s)], the kept predictions in table order.  events: what
        self.events(m, chan) returned (it is a loop over the universe: callers keep it)."""
        laugh, inv = self.laugh_and_invalid(m, chan)
        events = self.events(m, chan) if events is None else events
        preds = [(sm.to_frames(s), sm.to_frames(e)) for s, e in spans]
        per_pred = []
        for a, b in preds:
            pred = slice(a + 1, b + 1) if b > a else slice(0, 0)
            per_pred.append((int(np.count_nonzero(laugh[pred])), int(np.count_nonzero(~inv[pred]))))
        per_event = []
        for lo, hi in events:
            event = self.sets.oc(lo, hi)
            links = []
            for a, b in preds:
                ov = int(np.count_nonzero(event[a + 1:b + 1])) if b > a else 0
                if ov >= 1:
                    links.append((ov, a, b))
            per_event.append((lo, hi, links))
        return per_pred, per_event

    @staticmethod
    def score_pairs(pairs, min_overlap_ms=1, min_overlap_pct=0):
        """The seven integers of one channel and one setting from its pairs."""
        per_pred, per_event = pairs
        need = max(1, min_overlap_ms)
        pred_hit = sum(1 for lov, outside in per_pred if lov >= need and 100 * lov >= min_overlap_pct * outside)
        touched = hit = n_links = onset = offset = 0
        for lo, hi, links in per_event:
            cov = sum(ov for ov, _, _ in links)
            n_links += len(links)
            if len(links) >= 1:
                touched += 1
            if cov >= need and 100 * cov >= min_overlap_pct * (hi - lo):
                hit += 1
                onset += abs(links[0][1] - lo)
                offset += abs(links[-1][2] - hi)
        return (len(per_event), touched, hit, pred_hit, n_links, onset, offset)

    def score(self, spans, m, chan, min_overlap_ms=1, min_overlap_pct=0, events=None):
        return self.score_pairs(self.pairs(spans, m, chan, events), min_overlap_ms, min_overlap_pct)
