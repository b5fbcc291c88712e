"""TEST-ONLY restatement of the wide kinds of the per-window SystemRule exchange
(sentinel_amd/csrc/sf_sysx.h "the wide kinds", sf_engine.cpp ``sf_submit_node``
for a SystemRule with a thread, average-RT or firing load check) driven over
oracle engines, in the manner of tests/sysx_sim.py: plan windows, the binned
exit- and entry-side sums, the range classification, the level refinement, the
settled runs and q, against one replay of the whole node batch.

The rounds, the collectives and the forced sub-batches are restated here; the
plan step itself (``sxw_reduce`` with ``sxw_range`` and ``sys_classify``) and
the per-bin sums are the product's header, compiled on the host from
tests/sysx_wide_check.cpp (``-DSXW_SHARED``), which also checks them on its own
under the sanitizers.  As in sysx_sim, no entry counts as inert (that only
tightens a bound) and ENTRY_NODE is brought up to date by all-gathering the
round's decided IN events instead of the ranks' 16-word sums of them; a round
here always plans to the window's end, where the product limits a round's
range from the last q (fewer levels, the same verdicts)."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
from math import gcd

import numpy as np

from sentinel_amd import abi
from tests.sysx_sim import I64_MAX, I64_MIN, _BLOCKED, _allgather_i64

HERE = os.path.dirname(os.path.abspath(__file__))
SYS_NONE = 0xFF
DBL_MAX = 1.7976931348623157e308


class SimRule(C.Structure):
    _fields_ = [("qps", C.c_double), ("highest_load", C.c_double), ("highest_cpu", C.c_double),
                ("cur_load", C.c_double), ("cur_cpu", C.c_double), ("max_rt", C.c_int64), ("max_thread", C.c_int64)]


def build_lib(outdir) -> str:
    """The plan step as a host library under ``outdir`` (a temporary directory)."""
    so = os.path.join(str(outdir), "libsxw_sim.so")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-fPIC", "-shared", "-DSXW_SHARED",
                           "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-Wall",
                           "-Wno-unused-result", "-Wno-unused-value", "-Wno-unknown-pragmas", "-Wno-unused-function",
                           "-o", so, os.path.join(HERE, "sysx_wide_check.cpp")])
    return so


def load_lib(path: str):
    L = C.CDLL(path)
    L.sxw_c_plan_new.restype = C.c_void_p
    L.sxw_c_plan_free.argtypes = [C.c_void_p]
    L.sxw_c_begin.argtypes = [C.c_void_p, C.c_int64, C.c_int64]
    L.sxw_c_base.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int64, C.c_int64]
    L.sxw_c_ws_none.restype = C.c_int64
    L.sxw_c_stats.argtypes = [C.c_void_p] * 7 + [C.c_uint32, C.c_uint32, C.c_void_p, C.c_int64, C.c_void_p]
    L.sxw_c_reduce.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(SimRule), C.c_int, C.c_double,
                               C.c_void_p]
    L.sxw_c_rule_ok.argtypes = [C.POINTER(SimRule)]
    return L


def sim_rule(rules, status) -> SimRule:
    """sf_load_system_rules: the minimum of every set threshold."""
    r = SimRule(DBL_MAX, -1.0, -1.0, float(status[0]), float(status[1]), I64_MAX, I64_MAX)
    for x in rules:
        if x.highest_system_load >= 0:
            r.highest_load = x.highest_system_load if r.highest_load < 0 else min(r.highest_load, x.highest_system_load)
        if 0 <= x.highest_cpu_usage <= 1:
            r.highest_cpu = x.highest_cpu_usage if r.highest_cpu < 0 else min(r.highest_cpu, x.highest_cpu_usage)
        if x.avg_rt >= 0:
            r.max_rt = min(r.max_rt, x.avg_rt)
        if x.max_thread >= 0:
            r.max_thread = min(r.max_thread, x.max_thread)
        if x.qps >= 0:
            r.qps = min(r.qps, x.qps)
    return r


def submit_node_wide(o, L, batch: abi.HostBatch, seq: np.ndarray, comm, *, rule: SimRule, S: int, interval: int,
                     stat_max_rt: int = 5000, log: list | None = None) -> abi.HostVerdicts:
    """One rank of the exchange (sf_submit_node, wide kinds) over oracle engine ``o``.
    ``log`` gets one dict per round: the plan window's range, every level's
    (lo, hi, w, range of the next level or None), q, the settled runs, and what
    this rank's events of the sub-batch were."""
    n = batch.n
    seq = np.ascontiguousarray(seq, np.int64)
    wl = interval // S
    g = gcd(wl, 1000)
    isec = interval / 1000.0
    fl = np.ascontiguousarray(batch.flags, np.uint8)
    ts = np.ascontiguousarray(batch.ts_ms, np.int64)
    cnt = np.ascontiguousarray(batch.count, np.int32)
    eref = None if batch.entry_ref is None else np.ascontiguousarray(batch.entry_ref, np.int64)
    cts = None if batch.create_ts is None else np.ascontiguousarray(batch.create_ts, np.int64)
    is_ent = ((fl & abi.EV_IN) != 0) & ((fl & (abi.EV_EXIT | abi.EV_BLOCKED)) == 0)
    hdr = np.array([ts[0] // g if n else I64_MAX, ts[-1] // g if n else I64_MIN,
                    seq[-1] + 1 if n else I64_MIN, int((is_ent & (cnt < 0)).any()), n], np.int64)
    H = _allgather_i64(comm, hdr)
    live = H[:, 4] > 0
    assert not H[:, 3].any(), "negative acquireCount: the gather protocol"
    out = abi.HostVerdicts(n)
    if not live.any():
        return out
    C0, C1, seq_end = int(H[live, 0].min()), int(H[live, 1].max()), int(H[live, 2].max())
    nw = C1 - C0 + 1
    wf = np.full(nw, I64_MAX, np.int64)
    if n:
        cell = ts // g - C0
        first = np.r_[True, cell[1:] != cell[:-1]]
        wf[cell[first]] = seq[first]
    Wf = _allgather_i64(comm, wf).min(axis=0)
    wkey = np.nonzero(Wf != I64_MAX)[0]
    wseq = Wf[wkey]
    words, max_segs = L.sxw_c_words(), L.sxw_c_max_segs()
    plan = L.sxw_c_plan_new()
    segs = np.zeros((max_segs, 3), np.int64)
    po = np.zeros(8, np.int64)
    ws_none = L.sxw_c_ws_none()
    ptr = lambda a: None if a is None else a.ctypes.data        # noqa: E731
    lp, sp, j = 0, int(wseq[0]), 0
    pending = np.zeros((5, 0), np.int64)          # decided IN events of the last sub-batch: ts, c, flags, status, cts
    try:
        while True:
            fin = sp >= seq_end
            while not fin and j + 1 < wseq.size and wseq[j + 1] <= sp:
                j += 1
            # ENTRY_NODE += the node's IN events of the last sub-batch
            k_cnt = _allgather_i64(comm, np.array([pending.shape[1]], np.int64))[:, 0]
            pad = np.zeros((5, int(k_cnt.max())), np.int64)
            pad[:, :pending.shape[1]] = pending
            allp = _allgather_i64(comm, pad.reshape(-1)).reshape(len(k_cnt), 5, -1)
            ev = np.concatenate([allp[k][:, :k_cnt[k]] for k in range(len(k_cnt))], axis=1)
            if ev.shape[1]:
                m = ev.shape[1]
                o.entry_node_add(abi.HostBatch(np.zeros(m, np.uint32), ev[0], ev[1].astype(np.int32),
                                               ev[2].astype(np.uint8), entry_ref=np.full(m, -1, np.int64),
                                               create_ts=ev[4]), ev[3].astype(np.uint8))
            if fin:
                break
            lo, hi = sp, int(wseq[j + 1]) if j + 1 < wseq.size else seq_end
            wstart = (C0 + int(wkey[j])) * g
            en = o.read_entry_node()
            rows = np.array([[ws_none if en.second[i].window_start == abi.SF_WS_ABSENT else en.second[i].window_start,
                              en.second[i].pass_, en.second[i].success, en.second[i].rt, en.second[i].min_rt]
                             for i in range(S)], np.int64)
            L.sxw_c_begin(plan, lo, hi)
            L.sxw_c_base(plan, rows.ctypes.data, S, wl, interval, stat_max_rt, en.cur_thread_num, wstart)
            levels = []
            done = False
            cur = (lo, hi, (hi - lo + L.sxw_c_bins() - 1) // L.sxw_c_bins())
            while not done:
                msg = np.zeros(words, np.int64)
                L.sxw_c_stats(ts.ctypes.data, cnt.ctypes.data, fl.ctypes.data, ptr(eref), ptr(cts),
                              out.status.ctypes.data, seq.ctypes.data, n, lp, plan, rule.max_rt, msg.ctypes.data)
                msgs = np.ascontiguousarray(_allgather_i64(comm, msg))
                assert msgs.nbytes // msgs.shape[0] <= 16384
                L.sxw_c_reduce(msgs.ctypes.data, msgs.shape[0], plan, segs.ctypes.data, C.byref(rule), S, isec,
                               po.ctypes.data)
                done = bool(po[4])
                nxt = None if done else (int(po[0]), int(po[1]), int(po[2]))
                levels.append(dict(lo=cur[0], hi=cur[1], w=cur[2], next=nxt))
                cur = nxt
                assert len(levels) <= 66, "the plan did not converge"
            q, nseg = int(po[3]), int(po[6])
            assert sp < q <= hi and not po[7]
            lq = lp + int(np.searchsorted(seq[lp:], q))
            rec = dict(lo=lo, hi=hi, q=q, levels=levels, segs=segs[:nseg].copy(), lp=lp, lq=lq,
                       local_in_window=int(np.searchsorted(seq, hi) - np.searchsorted(seq, lo)),
                       local_entries=int(is_ent[int(np.searchsorted(seq, lo)):int(np.searchsorted(seq, hi))].sum()))
            if lq > lp:
                mask = np.full(lq - lp, SYS_NONE, np.uint8)
                ent = np.nonzero(is_ent[lp:lq])[0]
                if ent.size:
                    k = np.searchsorted(segs[:nseg, 0], seq[lp:lq][ent], side="right") - 1
                    assert (k >= 0).all() and (seq[lp:lq][ent] < segs[k, 1]).all(), "an entry before q in no settled run"
                    mask[ent] = segs[k, 2].astype(np.uint8)
                er = ct = None
                if eref is not None:
                    r = eref[lp:lq]
                    c0 = np.zeros(lq - lp, np.int64) if cts is None else cts[lp:lq].copy()
                    early = (r >= 0) & (r < lp)
                    rr = np.clip(r, 0, None)
                    er = np.where(r >= lp, r - lp, r)
                    er = np.where(early, np.where(np.isin(out.status[rr], _BLOCKED), -2, -1), er).astype(np.int64)
                    ct = np.where(early, ts[rr], c0).astype(np.int64)
                    x = (fl[lp:lq] & (abi.EV_IN | abi.EV_EXIT)) == (abi.EV_IN | abi.EV_EXIT)
                    rec.update(exits_earlier_round=int((x & early).sum()), exits_earlier_batch=int((x & (r == -1)).sum()),
                               exits_same_round=int((x & (r >= lp)).sum()),
                               exit_entry_seq=[(int(seq[lp + i]), int(seq[r[i]])) for i in np.nonzero(x & (r >= lp))[0]])
                kw = {}
                if batch.arg_tag is not None:
                    kw = dict(arg_tag=batch.arg_tag[:, lp:lq], arg_bits=batch.arg_bits[:, lp:lq],
                              n_args=None if batch.n_args is None else batch.n_args[lp:lq])
                sub = abi.HostBatch(batch.res_id[lp:lq], ts[lp:lq], cnt[lp:lq], fl[lp:lq], entry_ref=er, create_ts=ct,
                                    **kw)
                v = o.submit_forced(sub, mask)
                out.status[lp:lq], out.wait_ms[lp:lq], out.rule_idx[lp:lq] = v.status, v.wait_ms, v.rule_idx
                idx = np.nonzero((fl[lp:lq] & abi.EV_IN) != 0)[0] + lp
                c2 = np.zeros(idx.size, np.int64)
                if eref is not None:
                    r = eref[idx]
                    c2 = np.where(r >= 0, ts[np.clip(r, 0, None)], cts[idx] if cts is not None else ts[idx])
                pending = np.stack([ts[idx], cnt[idx].astype(np.int64), fl[idx].astype(np.int64),
                                    out.status[idx].astype(np.int64), c2])
            else:
                pending = np.zeros((5, 0), np.int64)
            if log is not None:
                log.append(rec)
            lp, sp = lq, q
    finally:
        L.sxw_c_plan_free(plan)
    assert lp == n
    return out
