"""Connections whose frames sit on the borders of sf_serve_frames' framing: the
16-KiB tiles of k_wire_exit / k_wire_walk (a tile of 8192 empty frames, the
longest path the 13 doublings must follow; length fields straddling a tile
edge; frames, connections and too-long frames starting and ending on offsets
16383 and 0), more connection starts in one tile than k_wire_walk has lanes,
total sizes of one and two tiles +- 1, and a connection handed to the host on
a tile edge.  Random traffic (tests/test_gpu_wire.py) reaches these only by
chance.

A case is a list of calls, each a list of connections' bytes; `carry` calls
take every connection's unconsumed remainder of the call before.  The guard is
a plain walk of the 2-byte lengths of each connection: it proves that the
promised offsets occur as frame / connection starts and ends, and that the
frames up to the ORACLE's `consumed` are as many as its `n_frames`.

Shared by tests/test_token_wire_cases.py (CPU) and
tests/test_gpu_token_wire_cases.py (the engine against the oracle).
"""
import os
import re
import struct

import numpy as np

from sentinel_amd import abi, trace, wire
from tests import token_cases as tc

T0 = trace.T0
_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ---- the engine's constants, restated (test_wire_constants_match_the_source) ----
WIRE_TILE = 16384           # sf_wire.h: bytes per framing tile
WIRE_ROUNDS = 13            # sf_wire.hip k_wire_exit: pointer doublings (2^13 hops >= 8192 frames of a tile)
WALK_LANES = 64             # sf_wire.hip k_wire_walk: entries walked at once
MAX_FRAME = 1024            # sentinel_flow.h SF_WIRE_MAX_FRAME

MIRROR = dict(WIRE_TILE=WIRE_TILE, WIRE_ROUNDS=WIRE_ROUNDS, WALK_LANES=WALK_LANES, MAX_FRAME=MAX_FRAME)


def source_constants(root=_ROOT):
    def text(*name):
        with open(os.path.join(root, *name)) as f:
            return f.read()

    def one(src, pat, n=1):
        m = re.findall(pat, src)
        assert len(m) == n, (pat, m)
        return m[0]
    wh, w, api = text("sentinel_amd", "csrc", "sf_wire.h"), text("sentinel_amd", "csrc", "sf_wire.hip"), \
        text("include", "sentinel_flow.h")
    out = {}
    out["WIRE_TILE"] = int(one(wh, r"constexpr uint32_t WIRE_TILE = (\d+);"))
    out["WIRE_ROUNDS"] = int(one(w, r"for \(int r = 0; r < (\d+); r\+\+\) \{"))
    out["WALK_LANES"] = int(one(w, r"__global__ void __launch_bounds__\((\d+)\) k_wire_walk\(WireBufs w\)"))
    out["MAX_FRAME"] = int(one(api, r"#define SF_WIRE_MAX_FRAME (\d+)"))
    # the byte after the tile (a straddling length field) is loaded by both kernels
    one(w, r"(const uint32_t lim = min\(len \+ 1, w\.n - base\);)", 2)
    one(w, r"(for \(uint32_t k = lane; k < n_ent; k \+= 64\) \{)")
    return out


FLOW_ID, PARAM_ID = 1, 2


def rules():
    return [tc.nsp(1, 1)], [tc.frule(FLOW_ID, 40)], [tc.prule(PARAM_ID, 5)]


# ---------------------------------------------------------------- frames
class Xid:
    def __init__(self):
        self.n = 0

    def __call__(self):
        self.n += 1
        return self.n


def f_empty(x):
    return wire.frame(b"")


def f_t9(x):
    return wire.frame(struct.pack(">ib", x(), 9))                       # no decoder, no data: 7 B, no response


def f_flow19(x):
    return wire.frame(struct.pack(">ibqi", x(), 1, FLOW_ID, 1))         # FLOW without the priority byte


def f_flow(x):
    return wire.flow_frame(x(), FLOW_ID, 1, x.n % 3 == 0)


def f_pstr(x):
    return wire.param_frame(x(), PARAM_ID, 1, [("str", "v%d" % (x.n % 4))])


def too_long(total):
    body = bytes((i * 7 + 3) & 0xff for i in range(total - 2))
    return struct.pack(">H", total - 2) + body


def f_long1100(x):
    return too_long(1100)


def f_long40000(x):
    return too_long(40000)


FILLERS = dict(empty=f_empty, t9=f_t9, flow19=f_flow19, flow=f_flow, pstr=f_pstr, long1100=f_long1100,
               long40000=f_long40000)


def s_short(x):
    return wire.frame(b"\x01\x02\x03")                                  # body of 3 bytes: decode() null, bytes stay


def s_ping(x):
    return wire.ping_frame(x(), "default")


def s_t9data(x):
    return wire.frame(struct.pack(">ib", x(), 9) + b"zz")


STOPPERS = dict(short=s_short, ping=s_ping, t9data=s_t9data)


class Layout:
    """Connections laid out back to back; offsets are those of the concatenated batch."""

    def __init__(self):
        self.streams = [bytearray()]
        self.x = Xid()

    def pos(self):
        return sum(len(s) for s in self.streams)

    def conn(self, data=b""):
        self.streams.append(bytearray(data))
        return len(self.streams) - 1

    def add(self, data):
        self.streams[-1] += data

    def put(self, kind):
        self.add(FILLERS[kind](self.x))

    def pad_to(self, off):
        """Frames of the current connection up to batch offset `off` exactly: too-long and FLOW
        frames while far, then a 7-byte frame if the rest is odd, and empty frames."""
        n = off - self.pos()
        assert n == 0 or n == 2 or n == 4 or n >= 6, n
        while n > 2300:
            self.add(too_long(1100) + f_flow(self.x) + f_pstr(self.x))
            n = off - self.pos()
        if n % 2:
            self.add(f_t9(self.x))
            n -= 7
        self.add(wire.frame(b"") * (n // 2))
        assert self.pos() == off

    def done(self):
        return [bytes(s) for s in self.streams]


class WireCase:
    def __init__(self, name):
        self.name = name
        self.calls = []         # (streams or None for carry, promises)

    def call(self, streams, **promises):
        self.calls.append((streams, promises))

    def carry(self, **promises):
        self.calls.append((None, promises))


def walk(streams, consumed=None):
    """Frame starts and ends (batch offsets) by the 2-byte lengths; with `consumed`, the number of
    frames before each connection's consumed prefix ends."""
    starts, ends, cstarts, cends = set(), set(), set(), set()
    handled = 0
    base = 0
    for s, data in enumerate(streams):
        if data:
            cstarts.add(base)
            cends.add(base + len(data))
        p = 0
        while p < len(data):
            if len(data) - p < 2:
                break
            n = (data[p] << 8) | data[p + 1]
            if p + 2 + n > len(data):
                break
            starts.add(base + p)
            ends.add(base + p + 2 + n)
            if consumed is not None and p < int(consumed[s]):
                handled += 1
            p += 2 + n
        base += len(data)
    return dict(start=starts, end=ends, cstart=cstarts, cend=cends, handled=handled, total=base)


def play(eng, case):
    """[(streams, WireResult, sums)]: load the rules, serve every call 3 s apart."""
    ns, flow, param = rules()
    eng.load_namespaces(ns)
    eng.load_cluster_rules(flow, param, [])
    out = []
    now = T0
    prev = None
    for streams, _ in case.calls:
        if streams is None:
            ins, r = prev
            streams = [s[int(r.consumed[k]):] for k, s in enumerate(ins)]
        r = eng.serve_frames(streams, now)
        sums = [tuple(int(eng.cluster_sum(FLOW_ID, ev, t)) for ev in range(7)) for t in (now, now + 999, now + 1000)]
        out.append((streams, r, sums))
        prev = (streams, r)
        now += 3000
    return out


def compare(case, got, want):
    assert len(got) == len(want) == len(case.calls)
    for k, ((gs, g, gsum), (ws, w, wsum)) in enumerate(zip(got, want)):
        what = f"{case.name} call {k}"
        assert gs == ws, what
        assert (g.n_frames, g.n_requests, g.n_responses) == (w.n_frames, w.n_requests, w.n_responses), \
            (what, (g.n_frames, g.n_requests, g.n_responses), (w.n_frames, w.n_requests, w.n_responses))
        assert np.array_equal(g.stop, w.stop), (what, "stop", np.nonzero(g.stop != w.stop)[0][:5])
        assert np.array_equal(g.consumed, w.consumed), (what, "consumed", np.nonzero(g.consumed != w.consumed)[0][:5])
        assert np.array_equal(g.resp_off, w.resp_off), (what, "resp_off")
        assert g.resp.shape == w.resp.shape and np.array_equal(g.resp, w.resp), (what, "resp")
        assert gsum == wsum, (what, gsum, wsum)


def guard(case, R):
    """On the oracle's results R."""
    notes = []
    for k, ((_, promises), (streams, r, _)) in enumerate(zip(case.calls, R)):
        w = walk(streams, r.consumed)
        assert w["handled"] == r.n_frames, (case.name, k, w["handled"], r.n_frames)
        for kind in ("start", "end", "cstart", "cend"):
            for off in promises.get(kind, ()):
                assert off in w[kind], (case.name, k, kind, off)
        if "total" in promises:
            assert w["total"] == promises["total"]
        for s, code in promises.get("stop", {}).items():
            assert r.stop[s] == code, (case.name, k, s, r.stop[s], code)
        for s, c in promises.get("consumed", {}).items():
            assert r.consumed[s] == c, (case.name, k, s, r.consumed[s], c)
        if "frames_in_tile0" in promises:
            assert sum(1 for x in w["start"] if x < WIRE_TILE) == promises["frames_in_tile0"]
        if promises.get("answers", True) and w["total"] > 40:
            assert r.n_responses > 0 and r.n_requests > 0, (case.name, k)
        notes.append(f"{r.n_frames}f/{r.n_responses}r")
    return " ".join(notes)


def tail(lay, n=3):
    for _ in range(n):
        lay.put("flow")
        lay.put("pstr")


# ---------------------------------------------------------------- 11. a tile of empty frames
def tile_of_empty_frames():
    c = WireCase("tile_of_empty_frames")
    lay = Layout()
    lay.add(wire.frame(b"") * (WIRE_TILE // 2))
    tail(lay)
    c.call(lay.done(), start=[WIRE_TILE - 2, WIRE_TILE], frames_in_tile0=WIRE_TILE // 2)
    lay = Layout()                                   # the same, shifted by one 7-byte frame
    lay.put("t9")
    lay.add(wire.frame(b"") * ((WIRE_TILE - 1 - 7) // 2))
    tail(lay)
    c.call(lay.done(), start=[WIRE_TILE - 1], frames_in_tile0=1 + (WIRE_TILE - 8) // 2 + 1)   # (+ the straddling one)
    lay = Layout()                                   # two connections of empty frames filling two tiles
    lay.add(wire.frame(b"") * (WIRE_TILE // 2 - 1))
    lay.conn(wire.frame(b"") * (WIRE_TILE // 2 + 1))
    lay.conn()
    tail(lay)
    c.call(lay.done(), cstart=[WIRE_TILE - 2, 2 * WIRE_TILE], start=[2 * WIRE_TILE - 2])
    return c


# ---------------------------------------------------------------- 12. start offsets
EDGE_OFFS = (WIRE_TILE - 3, WIRE_TILE - 2, WIRE_TILE - 1, 0, 1)


def start_offsets(kind, jump=False):
    """The filler starts on (jump: the 40000-byte frame jumps over two tiles and lands on) tile
    offsets 16381, 16382, 16383, 0 and 1 of two tiles."""
    c = WireCase(f"start_offsets[{kind}{'-lands' if jump else ''}]")
    tiles = (3, 4) if jump else (1, 2)
    targets = sorted(t * WIRE_TILE + o for t in tiles for o in EDGE_OFFS)
    if kind == "long40000":
        groups = [[t] for t in targets]
    else:
        groups = [targets[i::5] for i in range(5)]       # targets of one call lie more than a frame apart
    for g in groups:
        lay = Layout()
        lay.put("flow")
        for t in g:
            lay.pad_to(t - 40000 if jump else t)
            lay.put(kind)
            lay.put("flow")
        tail(lay, 1)
        c.call(lay.done(), **({"end": g, "start": [t - 40000 for t in g] + g} if jump else {"start": g}))
    return c


# ---------------------------------------------------------------- 13. frames and connections on the tile edge
def on_the_edge():
    c = WireCase("on_the_edge")
    E = WIRE_TILE
    lay = Layout()                                   # a frame and its connection end on the edge
    lay.pad_to(E - 20)
    lay.put("flow")
    lay.conn()
    tail(lay)
    c.call(lay.done(), end=[E], cend=[E], cstart=[E])
    lay = Layout()                                   # a connection starting on 16383
    lay.put("flow")
    lay.pad_to(E - 1)
    lay.conn()
    tail(lay)
    c.call(lay.done(), cstart=[E - 1], start=[E - 1])
    lay = Layout()                                   # a connection of 1 byte on 16383
    lay.put("flow")
    lay.pad_to(E - 1)
    lay.conn(b"\x00")
    lay.conn()
    tail(lay)
    c.call(lay.done(), cstart=[E - 1, E], stop={1: abi.WIRE_PARTIAL, 0: abi.WIRE_DONE, 2: abi.WIRE_DONE},
           consumed={1: 0})
    for cut, at in ((1, E - 1), (2, E - 1), (12, E - 4)):   # last frame: 1 byte, header only, body short
        lay = Layout()
        lay.put("flow")
        lay.pad_to(at)
        lay.add(f_flow(lay.x)[:cut])
        lay.conn()
        tail(lay)
        c.call(lay.done(), cend=[at + cut], stop={0: abi.WIRE_PARTIAL, 1: abi.WIRE_DONE}, consumed={0: at})
    lay = Layout()                                   # five edges, a different length byte behind each: the last
    lay.put("flow")                                  # frame of a connection starts on 16383 (complete if and
    for k, kind in enumerate(("empty", "t9", "flow19", "flow", "pstr")):    # only if that byte is read right)
        lay.pad_to((k + 1) * E - 1)
        lay.put(kind)
        lay.conn()
        lay.put("flow")
    lay.pad_to(6 * E - 1)
    lay.add(f_pstr(lay.x)[:2])                       # and a header alone: incomplete whatever the body length
    lay.conn()
    tail(lay)
    c.call(lay.done(), start=[k * E - 1 for k in range(1, 6)], cend=[E + 1, 2 * E + 6, 3 * E + 18, 4 * E + 19, 6 * E + 1],
           stop={0: abi.WIRE_DONE, 4: abi.WIRE_DONE, 5: abi.WIRE_PARTIAL}, consumed={5: 6 * E - 1 - (5 * E - 1 + 30)})
    for total, edge in ((1100, E), (40000, 3 * E)):  # a too-long frame ending with its connection on an edge
        lay = Layout()
        lay.put("flow")
        lay.pad_to(edge - total)
        lay.add(too_long(total))
        lay.conn()
        tail(lay)
        c.call(lay.done(), end=[edge], cend=[edge], stop={0: abi.WIRE_DONE})
    for total, have in ((1100, 700), (40000, 20000)):        # a too-long frame cut off by the connection's end
        lay = Layout()
        lay.put("flow")
        lay.pad_to(E - 300)
        lay.add(too_long(total)[:have])
        lay.conn()
        tail(lay)
        c.call(lay.done(), cend=[E - 300 + have], stop={0: abi.WIRE_PARTIAL}, consumed={0: E - 300})
    return c


# ---------------------------------------------------------------- 14. total sizes
TOTALS = (1, 2, WIRE_TILE - 1, WIRE_TILE, WIRE_TILE + 1, 2 * WIRE_TILE, 2 * WIRE_TILE + 1)


def total_sizes():
    c = WireCase("total_sizes")
    c.call([b"\x00"], total=1, stop={0: abi.WIRE_PARTIAL}, consumed={0: 0}, answers=False)
    c.call([wire.frame(b"")], total=2, stop={0: abi.WIRE_DONE}, consumed={0: 2}, answers=False)
    for total in TOTALS[2:]:
        lay = Layout()
        lay.put("flow")
        lay.pad_to(total - 20)
        lay.put("flow")
        c.call(lay.done(), total=total, end=[total], stop={0: abi.WIRE_DONE})
        lay = Layout()                               # the same size ending in a cut frame
        lay.put("flow")
        lay.pad_to(total - 7)
        lay.add(f_flow(lay.x)[:7])
        c.call(lay.done(), total=total, stop={0: abi.WIRE_PARTIAL}, consumed={0: total - 7})
    return c


# ---------------------------------------------------------------- 15. connection starts per tile
STARTS = (63, 64, 65, 130)


def connection_starts():
    """k non-empty connections starting in tile 1, behind the one continuing into it; empty
    connections between them and on both edges of the tile."""
    c = WireCase("connection_starts")
    for k in STARTS:
        lay = Layout()
        lay.put("flow")
        lay.pad_to(WIRE_TILE)
        lay.conn()                                   # an empty connection on the edge
        lay.conn()
        lay.put("flow")
        lay.pad_to(WIRE_TILE + 100)                  # this one starts on offset 0
        first = len(lay.streams)
        for i in range(k - 2):
            lay.conn()
            lay.put(("flow", "flow19", "pstr", "t9", "empty")[i % 5])
            if i % 4 == 0:
                lay.put("flow")
            if i % 3 == 0:
                lay.conn()                           # empty
        lay.conn()
        lay.put("flow")
        lay.pad_to(2 * WIRE_TILE)                    # the k-th start; ends on the edge
        lay.conn()
        lay.conn()
        tail(lay)
        streams = lay.done()
        in_tile = [s for s in range(len(streams))
                   if streams[s] and WIRE_TILE <= sum(len(x) for x in streams[:s]) < 2 * WIRE_TILE]
        assert len(in_tile) == k, (k, len(in_tile), first)
        c.call(streams, cstart=[WIRE_TILE, 2 * WIRE_TILE], cend=[WIRE_TILE, 2 * WIRE_TILE])
    return c


# ---------------------------------------------------------------- 16. HOST stop on a tile edge
def host_stop(kind):
    c = WireCase(f"host_stop[{kind}]")
    for at in (WIRE_TILE - 1, WIRE_TILE):
        lay = Layout()
        lay.put("flow")
        lay.pad_to(at)
        lay.add(STOPPERS[kind](lay.x))
        stop_len = lay.pos() - at
        lay.put("flow")
        lay.pad_to(2 * WIRE_TILE + 1000)             # requests behind the stop, in later tiles: not answered
        tail(lay)
        lay.conn()
        tail(lay)
        lay.conn(f_flow(lay.x)[:9])
        c.call(lay.done(), start=[at, at + stop_len], stop={0: abi.WIRE_HOST, 1: abi.WIRE_DONE, 2: abi.WIRE_PARTIAL},
               consumed={0: at, 2: 0})
        c.carry(stop={0: abi.WIRE_HOST, 1: abi.WIRE_DONE, 2: abi.WIRE_PARTIAL}, consumed={0: 0, 1: 0, 2: 0},
                answers=False)
    return c


def _cases():
    c = {}

    def add(make, *args):
        name = make.__name__ + ("[" + "-".join(str(a) for a in args) + "]" if args else "")
        c[name] = (lambda: make(*args))
    add(tile_of_empty_frames)
    for kind in FILLERS:
        add(start_offsets, kind)
    add(start_offsets, "long40000", True)
    add(on_the_edge)
    add(total_sizes)
    add(connection_starts)
    for kind in STOPPERS:
        add(host_stop, kind)
    return c


CASES = _cases()
