"""Front-end side of the API-gateway flow rules (sf_load_gateway_rules,
sf_gateway_args): what a gateway adapter keeps before and after the engine.

It holds the GatewayFlowRules in the iteration order of the Set given to
GatewayRuleManager.loadRules, interns the request items the rules read into
field ids (one per header / cookie / URL-parameter name, one for the client
IP, one for Host, one per regex rule), evaluates the regex rules
(GatewayRegexCache stays with the caller) and lays requests, their exits and
unrelated events out as one time-ordered sf_event_batch.  The engine parses
the items into ParamFlow arguments on the device (``FlowEngine.gateway_args``)
and decides the batch through the ordinary submit calls.
"""
from __future__ import annotations

import re
from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import abi

RESOURCE_MODE_ROUTE_ID, RESOURCE_MODE_CUSTOM_API_NAME = 0, 1
PARSE_CLIENT_IP, PARSE_HOST, PARSE_HEADER, PARSE_URL_PARAM, PARSE_COOKIE = 0, 1, 2, 3, 4
MATCH_EXACT, MATCH_PREFIX, MATCH_REGEX, MATCH_CONTAINS = 0, 1, 2, 3
NOT_MATCH_PARAM, DEFAULT_PARAM = "$NM", "$D"


def java_hash(s: str) -> int:
    """String.hashCode (over UTF-16 code units, wrapping int)."""
    h = 0
    raw = s.encode("utf-16-be", "surrogatepass")
    for k in range(0, len(raw), 2):
        h = (31 * h + ((raw[k] << 8) | raw[k + 1])) & 0xFFFFFFFF
    return h - (1 << 32) if h >= 1 << 31 else h


@dataclass
class ParamItem:
    """GatewayParamFlowItem."""
    parse_strategy: int
    field_name: Optional[str] = None
    pattern: Optional[str] = None
    match_strategy: int = MATCH_EXACT


@dataclass
class GatewayRule:
    """GatewayFlowRule (defaults as in the reference); ``resource`` is the
    engine's id of the route or API ``name``."""
    resource: int
    name: str
    resource_mode: int = RESOURCE_MODE_ROUTE_ID
    grade: int = abi.GRADE_QPS
    count: float = 0.0
    interval_sec: int = 1
    control_behavior: int = 0
    burst: int = 0
    max_queueing_timeout_ms: int = 500
    item: Optional[ParamItem] = None


def _blank(s) -> bool:
    return s is None or s.strip(" \t\n\x0b\f\r\x1c\x1d\x1e\x1f") == ""


class RuleTable:
    """The rules in Set iteration order with their field ids and patterns."""

    def __init__(self, rules):
        self.rules = list(rules)
        self.fields = {}          # key -> field id; key = (parse_strategy, field name or None[, regex pattern])
        self.regex = {}           # field id -> compiled pattern (a REGEX rule with a non-empty pattern)
        self.patterns = []
        self.c_rules = []
        pat_idx = {}
        for r in self.rules:
            c = abi.sf_gateway_rule(resource=r.resource, resource_hash=java_hash(r.name), resource_mode=r.resource_mode,
                                    grade=r.grade, count=r.count, interval_sec=r.interval_sec,
                                    control_behavior=r.control_behavior, burst=r.burst,
                                    max_queueing_timeout_ms=r.max_queueing_timeout_ms, has_item=int(r.item is not None),
                                    pattern=abi.GW_NONE)
            if r.item is not None:
                it = r.item
                c.parse_strategy, c.match_strategy = it.parse_strategy, it.match_strategy
                c.field_name_blank = int(_blank(it.field_name))
                if it.pattern is not None:
                    c.pattern = pat_idx.setdefault(it.pattern, len(self.patterns))
                    if c.pattern == len(self.patterns):
                        self.patterns.append(it.pattern)
                c.field_id = self._field(it)
            self.c_rules.append(c)

    def _field(self, it: ParamItem) -> int:
        name = it.field_name if it.parse_strategy in (PARSE_HEADER, PARSE_URL_PARAM, PARSE_COOKIE) else None
        key = (it.parse_strategy, name)
        if it.match_strategy == MATCH_REGEX and it.pattern:
            key += (it.pattern,)              # the flag of a request item belongs to one regex
        fid = self.fields.setdefault(key, len(self.fields))
        if len(key) == 3 and fid not in self.regex:
            self.regex[fid] = re.compile(it.pattern)
        return fid

    def load(self, engine):
        engine.load_gateway_rules(self.c_rules, self.patterns)

    def items_of(self, req: dict):
        """(field id, value, flags) of the request items the rules read and the
        request has.  req: client_ip, host, headers, params, cookies (str
        values; absent or None: the item is not there)."""
        out = []
        for key, fid in self.fields.items():
            parse, name = key[0], key[1]
            if parse == PARSE_CLIENT_IP:
                v = req.get("client_ip")
            elif parse == PARSE_HOST:
                v = req.get("host")
            elif parse in (PARSE_HEADER, PARSE_URL_PARAM, PARSE_COOKIE):
                v = (req.get({PARSE_HEADER: "headers", PARSE_URL_PARAM: "params", PARSE_COOKIE: "cookies"}[parse]) or {}).get(name)
            else:
                v = None                      # parseInternal's default: null
            if v is None:
                continue
            flags = 0
            if fid in self.regex and self.regex[fid].fullmatch(v) is None:     # Matcher.matches()
                flags = abi.GW_NOMATCH
            out.append((fid, v, flags))
        return out


def pack_requests(table: RuleTable, requests, ev_index) -> abi.HostGatewayBatch:
    """Requests (dicts: ts_ms, count, flags, entries [(resource id, mode), ...]
    and the items RuleTable.items_of reads) as one sf_gateway_batch."""
    res_off, val_off = [0], [0]
    res_id, res_mode, val_field, val_str, val_flags, strings = [], [], [], [], [], []
    seen = {}
    for q in requests:
        for r, m in q["entries"]:
            res_id.append(r); res_mode.append(m)
        res_off.append(len(res_id))
        for fid, v, fl in table.items_of(q):
            k = seen.setdefault(v, len(strings))
            if k == len(strings):
                strings.append(v)
            val_field.append(fid); val_str.append(k); val_flags.append(fl)
        val_off.append(len(val_field))
    str_off, data = abi.string_table(strings)
    return abi.HostGatewayBatch(ts_ms=[q["ts_ms"] for q in requests], count=[q.get("count", 1) for q in requests],
                                flags=[q.get("flags", abi.EV_IN) for q in requests], res_off=res_off, res_id=res_id,
                                res_mode=res_mode, val_off=val_off, val_field=val_field, val_str=val_str,
                                val_flags=val_flags, str_off=str_off, data=data, ev_index=ev_index)


def layout(table: RuleTable, requests, exits=(), extra=()):
    """One time-ordered event batch from requests, their exits and other events.

    exits: (ts_ms, request index, entry index of that request, extra flags such
    as EV_ERROR): an EXIT of a gateway entry of this batch; it takes the entry's
    resource, count and, through ``exit_pos``, its arguments.
    extra: dicts (ts_ms, res_id, count, flags and optionally create_ts, n_args,
    arg_tag [SF_MAX_ARGS], arg_bits [SF_MAX_ARGS]) the caller fills itself:
    unrelated events and the EXITs of earlier batches (entry_ref -1, with the
    arguments kept from that batch's columns).
    At equal times requests come first, then the extra events, then the exits.
    Returns (HostGatewayBatch, HostGatewayEvents, create_ts): after
    ``gateway_args`` ``events.batch(create_ts)`` is the batch to submit."""
    keys = [(q["ts_ms"], 0, i) for i, q in enumerate(requests)]
    keys += [(x["ts_ms"], 1, i) for i, x in enumerate(extra)]
    keys += [(x[0], 2, i) for i, x in enumerate(exits)]
    keys.sort()
    ev_index, pos_extra, pos_exit, n_total = [0] * len(requests), [0] * len(extra), [0] * len(exits), 0
    for _, kind, i in keys:
        if kind == 0:
            ev_index[i] = n_total
            n_total += len(requests[i]["entries"])
        else:
            (pos_extra if kind == 1 else pos_exit)[i] = n_total
            n_total += 1
    entry_ref = np.full(n_total, -1, np.int64)
    create_ts = np.zeros(n_total, np.int64)
    ev = abi.HostGatewayEvents(n_total, entry_ref, pos_exit)
    for x, p in zip(extra, pos_extra):
        ev.res_id[p], ev.ts_ms[p], ev.count[p], ev.flags[p] = x["res_id"], x["ts_ms"], x.get("count", 1), x["flags"]
        create_ts[p] = x.get("create_ts", 0)
        ev.n_args[p] = x.get("n_args", 0)
        if "arg_tag" in x:
            ev.arg_tag[:, p], ev.arg_bits[:, p] = x["arg_tag"], x["arg_bits"]
    for (ts, qi, k, fl), p in zip(exits, pos_exit):
        q = requests[qi]
        ev.res_id[p], ev.ts_ms[p], ev.count[p] = q["entries"][k][0], ts, q.get("count", 1)
        ev.flags[p] = abi.EV_EXIT | (q.get("flags", abi.EV_IN) & abi.EV_IN) | fl
        entry_ref[p] = ev_index[qi] + k
    return pack_requests(table, requests, ev_index), ev, create_ts
