package com.alibaba.csp.sentinel.gpu;

import java.lang.foreign.Arena;
import java.lang.foreign.MemoryLayout;
import java.lang.foreign.MemorySegment;
import java.lang.foreign.StructLayout;
import java.nio.charset.StandardCharsets;
import java.util.ArrayList;
import java.util.HashMap;
import java.util.List;
import java.util.Map;
import java.util.Set;
import java.util.function.ToIntFunction;
import java.util.regex.Pattern;

import com.alibaba.csp.sentinel.adapter.gateway.common.SentinelGatewayConstants;
import com.alibaba.csp.sentinel.adapter.gateway.common.rule.GatewayFlowRule;
import com.alibaba.csp.sentinel.adapter.gateway.common.rule.GatewayParamFlowItem;
import com.alibaba.csp.sentinel.util.StringUtil;

import static java.lang.foreign.ValueLayout.ADDRESS;
import static java.lang.foreign.ValueLayout.JAVA_BYTE;
import static java.lang.foreign.ValueLayout.JAVA_DOUBLE;
import static java.lang.foreign.ValueLayout.JAVA_INT;
import static java.lang.foreign.ValueLayout.JAVA_LONG;

/**
 * GatewayRuleManager's rules as the engine takes them (sf_load_gateway_rules), and what the
 * front-end keeps for sf_gateway_args: the rules in the iteration order of the Set given to
 * GatewayRuleManager.loadRules (the engine does not re-derive it), one field id per request
 * item the rules read (the client IP, Host, each header / URL-parameter / cookie name, and
 * one of its own per regex rule: the flag of a request item belongs to one regex), and the
 * compiled regexes, whose answer travels as SF_GW_NOMATCH in val_flags.
 *
 * The engine converts the rules (GatewayRuleManager.applyGatewayRuleInternal), evaluates the
 * converted ParamFlowRules ahead of the list of sf_load_param_rules (GatewayFlowSlot, order
 * -4000, before ParamFlowSlot) and parses the request items on the device; an embedder that
 * loads this table drops GatewayFlowSlot from its chain (INTEGRATION.md).
 */
final class GatewayRuleTable {
    static final int GW_NONE = 0xFFFFFFFF;            // sf_gateway_rule.pattern: null

    /** sf_gateway_rule: 72 bytes. */
    static final StructLayout GATEWAY_RULE = MemoryLayout.structLayout(
            JAVA_INT.withName("resource"), JAVA_INT.withName("resource_hash"),
            JAVA_INT.withName("resource_mode"), JAVA_INT.withName("grade"),
            JAVA_DOUBLE.withName("count"), JAVA_LONG.withName("interval_sec"),
            JAVA_INT.withName("control_behavior"), JAVA_INT.withName("burst"),
            JAVA_INT.withName("max_queueing_timeout_ms"), JAVA_INT.withName("has_item"),
            JAVA_INT.withName("parse_strategy"), JAVA_INT.withName("field_id"),
            JAVA_INT.withName("field_name_blank"), JAVA_INT.withName("match_strategy"),
            JAVA_INT.withName("pattern"), JAVA_INT.withName("pad"));

    /** sf_gateway_batch: the requests of one sf_gateway_args call. */
    static final StructLayout GATEWAY_BATCH = MemoryLayout.structLayout(
            JAVA_INT.withName("n"), JAVA_INT.withName("mem"),
            ADDRESS.withName("ts_ms"), ADDRESS.withName("count"), ADDRESS.withName("flags"),
            ADDRESS.withName("res_off"), ADDRESS.withName("res_id"), ADDRESS.withName("res_mode"),
            ADDRESS.withName("val_off"), ADDRESS.withName("val_field"), ADDRESS.withName("val_str"),
            ADDRESS.withName("val_flags"), ADDRESS.withName("str_off"), ADDRESS.withName("bytes"),
            JAVA_INT.withName("n_str"), MemoryLayout.paddingLayout(4),
            ADDRESS.withName("ev_index"));

    /** sf_gateway_events: the event columns the call fills (the arrays of the sf_event_batch to submit). */
    static final StructLayout GATEWAY_EVENTS = MemoryLayout.structLayout(
            JAVA_INT.withName("mem"), JAVA_INT.withName("n_total"),
            ADDRESS.withName("res_id"), ADDRESS.withName("ts_ms"), ADDRESS.withName("count"),
            ADDRESS.withName("flags"), ADDRESS.withName("n_args"), ADDRESS.withName("arg_tag"),
            ADDRESS.withName("arg_bits"), ADDRESS.withName("entry_ref"), ADDRESS.withName("exit_pos"),
            JAVA_INT.withName("n_exit"), MemoryLayout.paddingLayout(4));

    private final List<GatewayFlowRule> rules = new ArrayList<>();       // Set iteration order
    private final Map<String, Integer> fields = new HashMap<>();         // request item -> field id
    private final Map<Integer, Pattern> regex = new HashMap<>();         // field id of a regex rule -> its pattern
    private final Map<GatewayFlowRule, Integer> fieldOf = new HashMap<>();

    GatewayRuleTable(Set<GatewayFlowRule> conf) {
        if (conf != null) {
            for (GatewayFlowRule r : conf) {      // the order applyGatewayRuleInternal iterates in
                rules.add(r);
                if (r != null && r.getParamItem() != null) {
                    fieldOf.put(r, fieldId(r.getParamItem()));
                }
            }
        }
    }

    /** The id of the request item a rule reads; a REGEX rule with a pattern takes an id of its own. */
    private int fieldId(GatewayParamFlowItem item) {
        final int parse = item.getParseStrategy();
        final boolean named = parse == SentinelGatewayConstants.PARAM_PARSE_STRATEGY_HEADER
                || parse == SentinelGatewayConstants.PARAM_PARSE_STRATEGY_URL_PARAM
                || parse == SentinelGatewayConstants.PARAM_PARSE_STRATEGY_COOKIE;
        String key = parse + "\u0000" + (named ? item.getFieldName() : "");
        final boolean isRegex = item.getMatchStrategy() == SentinelGatewayConstants.PARAM_MATCH_STRATEGY_REGEX
                && StringUtil.isNotEmpty(item.getPattern());
        if (isRegex) {
            key += "\u0000" + item.getPattern();
        }
        Integer id = fields.get(key);
        if (id == null) {
            id = fields.size();
            fields.put(key, id);
            if (isRegex) {
                regex.put(id, Pattern.compile(item.getPattern()));      // GatewayRegexCache stays with the caller
            }
        }
        return id;
    }

    /** Field id of the item rule {@code r} reads (for packing val_field). */
    int fieldOf(GatewayFlowRule r) {
        return fieldOf.get(r);
    }

    /** val_flags of a present request item: SF_GW_NOMATCH when the field is a regex rule's and the value does not match. */
    byte flagsOf(int fieldId, String value) {
        final Pattern p = regex.get(fieldId);
        return p != null && !p.matcher(value).matches() ? SentinelFlowNative.GW_NOMATCH : 0;
    }

    /** arg_bits of a String argument (sf_gateway_string_bits): FNV-1a 64 of its UTF-8 bytes. */
    static long stringBits(String s) {
        long h = 0xcbf29ce484222325L;
        for (byte b : s.getBytes(StandardCharsets.UTF_8)) {
            h = (h ^ (b & 0xFF)) * 0x100000001b3L;
        }
        return h;
    }

    /** sf_load_gateway_rules with the rules in Set iteration order (an empty table clears the gateway list). */
    void load(MemorySegment engine, ToIntFunction<String> resourceId) {
        final int n = rules.size();
        final List<byte[]> patterns = new ArrayList<>();
        final Map<String, Integer> patternIdx = new HashMap<>();
        try (Arena a = Arena.ofConfined()) {
            final long stride = GATEWAY_RULE.byteSize();
            final MemorySegment table = a.allocate(Math.max(1, n) * stride, 8);
            for (int k = 0; k < n; k++) {
                final GatewayFlowRule r = rules.get(k);
                final MemorySegment s = table.asSlice(k * stride, stride);
                final boolean blank = r == null || StringUtil.isBlank(r.getResource());
                s.set(JAVA_INT, o("resource"), blank ? 0 : resourceId.applyAsInt(r.getResource()));
                s.set(JAVA_INT, o("resource_hash"), blank ? 0 : r.getResource().hashCode());
                // a null rule or a blank resource is invalid in the reference: a negative mode makes it so here
                s.set(JAVA_INT, o("resource_mode"), blank ? -1 : r.getResourceMode());
                if (r == null) {
                    continue;
                }
                s.set(JAVA_INT, o("grade"), r.getGrade());
                s.set(JAVA_DOUBLE, o("count"), r.getCount());
                s.set(JAVA_LONG, o("interval_sec"), r.getIntervalSec());
                s.set(JAVA_INT, o("control_behavior"), r.getControlBehavior());
                s.set(JAVA_INT, o("burst"), r.getBurst());
                s.set(JAVA_INT, o("max_queueing_timeout_ms"), r.getMaxQueueingTimeoutMs());
                final GatewayParamFlowItem item = r.getParamItem();
                s.set(JAVA_INT, o("has_item"), item == null ? 0 : 1);
                s.set(JAVA_INT, o("pattern"), GW_NONE);
                if (item == null) {
                    continue;
                }
                s.set(JAVA_INT, o("parse_strategy"), item.getParseStrategy());
                s.set(JAVA_INT, o("field_id"), fieldOf.get(r));
                s.set(JAVA_INT, o("field_name_blank"), StringUtil.isBlank(item.getFieldName()) ? 1 : 0);
                s.set(JAVA_INT, o("match_strategy"), item.getMatchStrategy());
                if (item.getPattern() != null) {
                    Integer p = patternIdx.get(item.getPattern());
                    if (p == null) {
                        p = patterns.size();
                        patternIdx.put(item.getPattern(), p);
                        patterns.add(item.getPattern().getBytes(StandardCharsets.UTF_8));
                    }
                    s.set(JAVA_INT, o("pattern"), p);
                }
            }
            final MemorySegment strOff = a.allocate((patterns.size() + 1) * 4L, 4);
            int total = 0;
            for (int i = 0; i < patterns.size(); i++) {
                strOff.setAtIndex(JAVA_INT, i, total);
                total += patterns.get(i).length;
            }
            strOff.setAtIndex(JAVA_INT, patterns.size(), total);
            final MemorySegment bytes = a.allocate(Math.max(1, total), 1);
            long at = 0;
            for (byte[] p : patterns) {
                MemorySegment.copy(p, 0, bytes, JAVA_BYTE, at, p.length);
                at += p.length;
            }
            SentinelFlowNative.check((int) SentinelFlowNative.LOAD_GATEWAY.invokeExact(engine, table, n, strOff, bytes,
                    patterns.size()));
        } catch (RuntimeException | Error e) {
            throw e;
        } catch (Throwable t) {
            throw new IllegalStateException(t);
        }
    }

    /** Byte offset of a field of sf_gateway_rule. */
    private static long o(String field) {
        return SentinelFlowNative.off(GATEWAY_RULE, field);
    }
}
