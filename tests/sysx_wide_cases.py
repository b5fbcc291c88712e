"""Workloads of the wide kinds of the SystemRule exchange (sf_sysx.h): node
batches under a SystemRule with a thread, average-RT or firing load check, for
tests/test_system_exchange_wide.py (CPU restatement and GPU engines alike).

``workload(kind)`` -> (w, batches).  The border cases are a few hundred events
each over 8 resources without flow rules, under a thread rule, so that every
entry's outcome is plain arithmetic: entry k of a run of entries reads
``threads = (passed entries before it) - (exits before it)``.  Plan windows are
the 500-ms cells of the default geometry; the exchange's wide format has
BINS = 64 bins per level."""
import numpy as np

from sentinel_amd import abi
from tests import workloads

BINS = 64
IN, EXIT = abi.EV_IN, abi.EV_IN | abi.EV_EXIT


def _rule(qps=-1.0, avg_rt=-1, max_thread=-1, load=-1.0, cpu=-1.0):
    return [abi.sf_system_rule(highest_system_load=load, highest_cpu_usage=cpu, qps=qps, avg_rt=avg_rt,
                               max_thread=max_thread)]


# thresholds of the combined rule, picked with the oracle on this traffic so
# that each of the three reasons occurs (asserted where the reference is made)
COMBINED = dict(qps=4000.0, avg_rt=20, max_thread=3500)


def workload(kind):
    if kind in ("thread", "rt", "load"):
        w = workloads.system(kind)
        return w, w["batches"]
    if kind == "combined":
        w = workloads.system("thread")
        w["system"] = _rule(**COMBINED)
        return w, w["batches"]
    if kind == "geom":                                     # one bucket of 1500 ms: plan windows of 500 ms, 3 per bucket
        w = workloads.system("thread")
        c = w["cfg"]
        w["cfg"] = abi.default_config(max_resources=c.max_resources, max_batch=c.max_batch, sample_count=1,
                                      interval_ms=1500)
        w["system"] = _rule(max_thread=3000, avg_rt=40)
        return w, w["batches"]
    return border(kind)


class _Stream:
    """Events appended in submission order; exits name their entry's index."""

    def __init__(self):
        self.res, self.ts, self.cnt, self.fl, self.ref = [], [], [], [], []

    def entry(self, res, t, c=1):
        self.res.append(res); self.ts.append(t); self.cnt.append(c); self.fl.append(IN); self.ref.append(-1)
        return len(self.res) - 1

    def exit(self, entry, t):
        self.res.append(self.res[entry]); self.ts.append(t); self.cnt.append(self.cnt[entry]); self.fl.append(EXIT)
        self.ref.append(entry)
        return len(self.res) - 1

    def batch(self):
        return abi.HostBatch(np.array(self.res, np.uint32), np.array(self.ts, np.int64), np.array(self.cnt, np.int32),
                             np.array(self.fl, np.uint8), entry_ref=np.array(self.ref, np.int64),
                             create_ts=np.zeros(len(self.res), np.int64))


BORDERS = ("few", "bins_plus_one", "last_bin", "same_bin", "earlier_round", "earlier_batch", "only_exits",
           "idle_rank", "empty_batch")


def border(kind, world=2):
    """(w, batches) of one border of the wide plan step; see the guards in
    tests/test_system_exchange_wide.py for what each must reach."""
    R = 8
    s = _Stream()
    cuts = None
    max_thread = 10
    even = [r for r in range(R) if r % world == 0]
    if kind == "few":                          # a plan window with fewer sequence numbers than bins
        for k in range(20):
            s.entry(k % R, 1000 + k)
        for k in range(200):
            s.entry(k % R, 1600 + k)
    elif kind == "bins_plus_one":              # a plan window with exactly BINS + 1
        for k in range(BINS + 1):
            s.entry(k % R, 1000 + k)
        for k in range(100):
            s.entry(k % R, 1500 + k)
        max_thread = 40
    elif kind == "last_bin":                   # 2 * BINS entries, the limit crossed at the very last one
        for k in range(2 * BINS):
            s.entry(k % R, 1000 + k)
        for k in range(60):
            s.entry(k % R, 1500 + k)
        max_thread = 2 * BINS - 2
    elif kind == "same_bin":                   # entry and exit in one bin of the first level (width 4)
        open_ = []
        for k in range(4 * BINS):
            if k % 4 == 1:
                s.exit(open_.pop(), 1000 + k)
            else:
                open_.append(s.entry(k % R, 1000 + k))
        max_thread = 60
    elif kind in ("earlier_round", "earlier_batch"):
        # the limit is reached, rounds end there, and the exits that follow free threads again
        open_ = []
        for k in range(30):
            open_.append(s.entry(k % R, 1000 + k))
        for rep in range(6):
            for k in range(8):
                s.exit(open_.pop(0), 1100 + 40 * rep + k)
            for k in range(12):
                open_.append(s.entry((k + rep) % R, 1100 + 40 * rep + 10 + k))
        if kind == "earlier_batch":
            cuts = [0, 60, len(s.res)]
        max_thread = 12
    elif kind == "only_exits":                 # a plan window that holds nothing but exits
        open_ = [s.entry(k % R, 1000 + k) for k in range(40)]
        for k in range(25):
            s.exit(open_.pop(0), 1600 + k)
        for k in range(60):
            s.entry(k % R, 2100 + k)
        max_thread = 25
    elif kind == "idle_rank":                  # a plan window in which one rank has no event
        for k in range(60):
            s.entry(k % R, 1000 + k)
        for k in range(60):
            s.entry(even[k % len(even)], 1600 + k)
        for k in range(60):
            s.entry(k % R, 2100 + k)
        max_thread = 100
    elif kind == "empty_batch":                # a node batch in which one rank has no event at all
        for k in range(60):
            s.entry(k % R, 1000 + k)
        for k in range(60):
            s.entry(even[k % len(even)], 1100 + k)
        for k in range(60):
            s.entry(k % R, 1200 + k)
        cuts = [0, 60, 120, 180]
        max_thread = 100
    else:
        raise KeyError(kind)
    full = s.batch()
    cuts = cuts or [0, full.n]
    batches = [full.subset(a, b) for a, b in zip(cuts[:-1], cuts[1:])]
    w = dict(cfg=abi.default_config(max_resources=R, max_batch=full.n), system=_rule(max_thread=max_thread),
             status=(0.0, 0.0))
    return w, batches
