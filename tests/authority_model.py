"""TEST-ONLY restatement of the reference's AuthorityRule classes over strings
(sentinel-core/.../slots/block/authority/): the expectation of the engine's
AuthorityRule tests.  No engine code is used here.

  AuthorityRuleChecker.passCheck            AuthorityRuleChecker.java:30-71
  AuthorityRuleManager.loadAuthorityConf    AuthorityRuleManager.java:108-139
  AuthorityRuleManager.isValidRule          AuthorityRuleManager.java:147-150
  AuthoritySlot.checkBlackWhiteAuthority    AuthoritySlot.java:51-70
"""
from dataclasses import dataclass
from typing import Optional

import numpy as np

AUTHORITY_WHITE, AUTHORITY_BLACK = 0, 1          # RuleConstant.java
ORIGIN_NONE = 0xFFFFFFFF                         # SF_ORIGIN_NONE: the empty origin ""


@dataclass
class AuthorityRule:
    """AuthorityRule.java: resource, limitApp (comma-separated), strategy (default AUTHORITY_WHITE)."""
    resource: Optional[str] = None
    limit_app: Optional[str] = None
    strategy: int = AUTHORITY_WHITE


def _is_blank(s) -> bool:                        # StringUtil.isBlank: null, empty or whitespace only
    return s is None or s.strip() == ""


def is_valid_rule(rule) -> bool:
    """AuthorityRuleManager.isValidRule (:147-150)."""
    return rule is not None and not _is_blank(rule.resource) and rule.strategy >= 0 and not _is_blank(rule.limit_app)


def _java_split(s: str):
    """String.split(","): trailing empty strings are removed."""
    parts = s.split(",")
    while parts and parts[-1] == "":
        parts.pop()
    return parts


def pass_check(rule: AuthorityRule, origin: Optional[str]) -> bool:
    """AuthorityRuleChecker.passCheck (:30-71)."""
    if not origin or not rule.limit_app:                          # :36 StringUtil.isEmpty
        return True
    contain = rule.limit_app.find(origin) > -1                    # :42-43
    if contain:                                                   # :46-57
        contain = any(origin == app for app in _java_split(rule.limit_app))
    if rule.strategy == AUTHORITY_BLACK and contain:              # :61
        return False
    if rule.strategy == AUTHORITY_WHITE and not contain:          # :66
        return False
    return True


class AuthorityRuleManager:
    """The rule map: resource -> the one rule kept for it."""

    def __init__(self):
        self.rules = {}

    def load_rules(self, rules):
        """loadAuthorityConf (:108-139): a load replaces the map; null or an
        empty list clears it; invalid rules are ignored; of the rules of one
        resource the first valid one is kept."""
        new = {}
        for r in rules or []:
            if not is_valid_rule(r):
                continue
            if r.resource not in new:
                new[r.resource] = r
        self.rules = new

    def get_rules(self):
        return list(self.rules.values())

    def blocks(self, resource: str, origin: Optional[str]) -> bool:
        """AuthoritySlot.checkBlackWhiteAuthority (:51-70) throws AuthorityException."""
        r = self.rules.get(resource)
        return r is not None and not pass_check(r, origin)


class Interner:
    """The caller's string interner of origins and limitApp pieces: "default"
    0, "other" 1, "" ORIGIN_NONE, every other string the next id."""

    def __init__(self):
        self.ids = {"default": 0, "other": 1, "": ORIGIN_NONE}
        self.names = {0: "default", 1: "other", ORIGIN_NONE: ""}
        self.next = 2

    def id(self, s: str) -> int:
        if s not in self.ids:
            while self.next in self.names:
                self.next += 1
            self.ids[s] = self.next
            self.names[self.next] = s
        return self.ids[s]

    def name(self, k: int) -> str:
        """The string of an id; an id a workload made up gets the name "app#<id>"."""
        k = int(k)
        if k not in self.names:
            self.names[k] = f"app#{k}"
            self.ids[self.names[k]] = k
        return self.names[k]


def to_tables(rules, res_id, interner: Interner):
    """What a caller hands to the engine for a rule list: (resource id,
    strategy, [origin ids]) per rule, in list order.  limitApp is split at ","
    without trimming; a blank limitApp is an empty list, a blank resource
    0xFFFFFFFF (both invalid).  ``res_id``: resource name -> id."""
    out = []
    for r in rules:
        if r is None:
            continue
        res = 0xFFFFFFFF if _is_blank(r.resource) else res_id(r.resource)
        ids = [] if _is_blank(r.limit_app) else [interner.id(p) for p in r.limit_app.split(",")]
        out.append((res, r.strategy, ids))
    return out


def blocked_mask(mgr: AuthorityRuleManager, res_name, res_ids, origin_ids, flags, interner: Interner, ev_exit=0x01,
                 ev_blocked=0x10) -> np.ndarray:
    """The entries of a batch that AuthoritySlot blocks: not exits (exits are
    untouched, AuthoritySlot.java:46-49), not entries the caller already
    flagged.  Decided per distinct (resource, origin) pair, on strings."""
    res_ids = np.asarray(res_ids, np.uint32)
    origin_ids = np.asarray(origin_ids, np.uint32)
    key = res_ids.astype(np.uint64) << np.uint64(32) | origin_ids.astype(np.uint64)
    uniq, inv = np.unique(key, return_inverse=True)
    verdict = np.array([mgr.blocks(res_name(int(k >> np.uint64(32))), interner.name(int(k & np.uint64(0xFFFFFFFF))))
                        for k in uniq], bool)
    ent = (np.asarray(flags) & (ev_exit | ev_blocked)) == 0
    return verdict[inv] & ent
