"""TEST-ONLY helpers of the AuthorityRule GPU tests (tests/test_gpu_authority.py):
origin columns for workloads that have none, rule lists that block a chosen
share of a workload's entries, and the expectation of a batch -- the string
model (tests/authority_model.py) marks the entries, the oracle replays the
batch with those entries flagged EV_BLOCKED, and its verdict 9 (V_BLOCK_OTHER)
becomes 10 (V_BLOCK_AUTHORITY) at the marked positions.  No engine code here."""
import copy

import numpy as np

from sentinel_amd import abi
from tests import authority_model as am


def res_name(r: int) -> str:
    return f"res{int(r)}"


def res_id(name: str) -> int:
    return int(name[3:])


def hashed_origins(b: abi.HostBatch, n_origins=8, seed=0, none_frac=0.2) -> np.ndarray:
    """An origin id per event, a hash of (resource, the entry's time): an exit
    carries its entry's origin also when the entry lies in an earlier batch
    (create_ts).  Ids 2 .. n_origins + 1, or ORIGIN_NONE."""
    t = b.ts_ms.copy()
    if b.entry_ref is not None:
        ex = (b.flags & abi.EV_EXIT) != 0
        inb = ex & (b.entry_ref >= 0)
        t[inb] = b.ts_ms[b.entry_ref[inb]]
        if b.create_ts is not None:
            early = ex & (b.entry_ref < 0)
            t[early] = b.create_ts[early]
    h = (b.res_id.astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15)) ^ (t.astype(np.uint64) * np.uint64(0xC2B2AE3D27D4EB4F))
    h ^= np.uint64((seed * 0x165667B19E3779F9 + 7) % (1 << 64))
    h ^= h >> np.uint64(29)
    h *= np.uint64(0xBF58476D1CE4E5B9)
    h ^= h >> np.uint64(32)
    og = (np.uint64(2) + h % np.uint64(n_origins)).astype(np.uint32)
    og[((h >> np.uint64(40)) % np.uint64(1000)) < np.uint64(int(none_frac * 1000))] = abi.ORIGIN_NONE
    return og


def add_origins(w, n_origins=8, seed=0, none_frac=0.2):
    """The workload with hashed_origins on every batch."""
    for b in w["batches"]:
        b.origin = hashed_origins(b, n_origins, seed, none_frac)
    return w


def pick_rules(batches, R, it: am.Interner, seed=0, share=0.10, listed=1, hot=None):
    """White and black AuthorityRules on about ``share`` of the resources, the
    busiest ones included (``hot`` of them, default half): a black list names
    ``listed`` of the origins the traffic carries, a white list all but
    ``listed`` of them.  Returns the string rule list."""
    rng = np.random.default_rng(seed)
    res = np.concatenate([b.res_id for b in batches])
    og = np.concatenate([b.origin for b in batches])
    ids = np.unique(og[og != abi.ORIGIN_NONE])
    names = [it.name(k) for k in ids]
    per = np.bincount(res, minlength=R)
    k = max(2, int(round(R * share)))
    hot = k // 2 if hot is None else hot
    order = np.argsort(-per, kind="stable")
    chosen = list(order[:hot]) + list(rng.choice(order[hot:], size=k - hot, replace=False))
    rules = []
    for i, r in enumerate(chosen):
        pick = set(rng.choice(len(names), size=min(listed, len(names) - 1), replace=False).tolist())
        if i % 2 == 0:
            rules.append(am.AuthorityRule(res_name(r), ",".join(names[j] for j in sorted(pick)), am.AUTHORITY_BLACK))
        else:
            rules.append(am.AuthorityRule(res_name(r), ",".join(n for j, n in enumerate(names) if j not in pick),
                                          am.AUTHORITY_WHITE))
    return rules


def marks_of(mgr: am.AuthorityRuleManager, b: abi.HostBatch, it: am.Interner) -> np.ndarray:
    if b.origin is None:
        return np.zeros(b.n, bool)
    return am.blocked_mask(mgr, res_name, b.res_id, b.origin, b.flags, it, abi.EV_EXIT, abi.EV_BLOCKED)


def share_of(mgr, batches, it) -> float:
    ent = sum(int(((b.flags & abi.EV_EXIT) == 0).sum()) for b in batches)
    return sum(int(marks_of(mgr, b, it).sum()) for b in batches) / max(ent, 1)


def split_for(mgr, b: abi.HostBatch, it):
    """(engine batch, oracle batch, marks) of one batch under the map in force.
    An exit whose entry lay in an earlier batch (entry_ref -1, create_ts) and
    was blocked there carries entry_ref -2 in both, as a caller that saw the
    entry's verdict would send it; the oracle's copy has the marked entries
    flagged EV_BLOCKED."""
    mark = marks_of(mgr, b, it)
    eb = copy.copy(b)
    if b.entry_ref is not None and b.create_ts is not None and b.origin is not None:
        early = ((b.flags & abi.EV_EXIT) != 0) & (b.entry_ref == -1)
        would = am.blocked_mask(mgr, res_name, b.res_id, b.origin, np.zeros(b.n, np.uint8), it)
        dead = early & would
        if dead.any():
            eb.entry_ref = b.entry_ref.copy()
            eb.entry_ref[dead] = -2
    ob = copy.copy(eb)
    ob.flags = eb.flags.copy()
    ob.flags[mark] |= abi.EV_BLOCKED
    return eb, ob, mark


def expected(want: abi.HostVerdicts, mark: np.ndarray) -> abi.HostVerdicts:
    """The oracle's verdicts of the pre-flagged batch with 9 turned into 10 at the marked positions."""
    assert (want.status[mark] == abi.V_BLOCK_OTHER).all()
    want.status[mark] = abi.V_BLOCK_AUTHORITY
    return want


def blocked_pairs(batches, marks, limit=48):
    """(resource, origin) pairs of marked entries, the most frequent first."""
    keys = np.concatenate([b.res_id[m].astype(np.uint64) << np.uint64(32) | b.origin[m].astype(np.uint64)
                           for b, m in zip(batches, marks)] or [np.zeros(0, np.uint64)])
    u, c = np.unique(keys, return_counts=True)
    top = u[np.argsort(-c, kind="stable")[:limit]]
    return [(int(k >> np.uint64(32)), int(k & np.uint64(0xFFFFFFFF))) for k in top]
