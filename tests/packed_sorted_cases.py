"""Workloads for the packed sorted-event word (sf_decide.h ev_pack / ev_*):
batches whose events need the word's two escapes.  A time offset of 65,535 ms
or more from the batch's first event, and an acquireCount outside 1..255, are
read from the caller's batch through the sort permutation.

Built from the generators of tests/workloads.py; shared by the CPU validity
test (oracle alone) and the GPU parity test.
"""
import numpy as np

from sentinel_amd import abi, trace
from tests import workloads

FAR_MS = 65_535                       # PV_DTS_FAR: first offset the word cannot hold
ODD_COUNTS = (0, 255, 256, 70_000, -1)


def stretch(w, k, system_qps_scale=True):
    """The workload with every time offset from T0 multiplied by k (order and
    ties between distinct times preserved; create_ts likewise)."""
    for b in w["batches"]:
        b.ts_ms = (b.ts_ms - trace.T0) * k + trace.T0
        if b.create_ts is not None:
            b.create_ts = np.where(b.create_ts > 0, (b.create_ts - trace.T0) * k + trace.T0, b.create_ts)
    if system_qps_scale and w.get("system"):
        for r in w["system"]:
            if r.qps > 0:
                r.qps = r.qps / k     # the same fraction of the offered rate
    return w


def long_single():
    """One batch of 200 s: most events past the 16-bit offset; THREAD exits
    near their entry and (capped at the batch's end) far from it."""
    return workloads.config3(R=2000, n=80_000, split=1, duration_ms=200_000)


def boundary():
    """One batch of 66 s: the offset boundary falls inside the segments."""
    return workloads.config3(R=2000, n=80_000, split=1, duration_ms=66_000)


def counts(seed=77, frac=0.05):
    """config3 at its default duration with a seeded 5 % of the entries given
    acquireCounts from ODD_COUNTS; an exit keeps its entry's count."""
    w = workloads.config3(R=2000, n=80_000, split=1)
    b = w["batches"][0]
    rng = np.random.default_rng(seed)
    cnt = b.count.copy()
    ent = np.nonzero((b.flags & abi.EV_EXIT) == 0)[0]
    pick = ent[rng.random(ent.size) < frac]
    cnt[pick] = rng.choice(np.array(ODD_COUNTS, np.int32), size=pick.size)
    ex = np.nonzero(((b.flags & abi.EV_EXIT) != 0) & (b.entry_ref >= 0))[0]
    cnt[ex] = cnt[b.entry_ref[ex]]
    b.count = cnt
    return w


def system_views():
    """SystemRule sub-batch views (base != 0) over 72 s: the escapes gather
    through a view's offset pointers."""
    return stretch(workloads.system("qps"), 18)


def xflow_long():
    return workloads.xflow(n=40_000, duration_ms=70_000, split=1)


def param_long():
    return stretch(workloads.param_mixed(), 12)


CASES = {
    "long_single": long_single, "boundary": boundary, "counts": counts, "system_views": system_views,
    "xflow_long": xflow_long, "param_long": param_long,
}
# cases whose point is the time escape: the span one batch must exceed
FAR_CASES = ("long_single", "boundary", "system_views", "xflow_long", "param_long")
