package com.alibaba.csp.sentinel.gpu;

import java.lang.foreign.Arena;
import java.lang.foreign.MemoryLayout;
import java.lang.foreign.MemorySegment;
import java.lang.foreign.StructLayout;
import java.util.ArrayList;
import java.util.List;
import java.util.function.ToIntFunction;

import com.alibaba.csp.sentinel.slots.block.authority.AuthorityRule;
import com.alibaba.csp.sentinel.util.StringUtil;

import static java.lang.foreign.ValueLayout.JAVA_INT;

/**
 * AuthorityRuleManager's rule list as the engine takes it (sf_load_authority_rules): one
 * sf_authority_rule per rule in list order, limitApp split at "," exactly as
 * AuthorityRuleChecker.passCheck splits it (no trimming) and each piece interned with the
 * interner of the event origins.  Validity and "the first valid rule of a resource wins"
 * are the engine's (AuthorityRuleManager.loadAuthorityConf): a blank resource goes as
 * 0xFFFFFFFF, a blank limitApp as an empty list.
 *
 * GpuFlowSlot still runs the reference AuthoritySlot itself and flags what it blocks
 * SF_EV_BLOCKED (verdict V_BLOCK_OTHER); an embedder that loads this table instead drops
 * that call and reads V_BLOCK_AUTHORITY.
 */
final class AuthorityRuleTable {
    /** sf_authority_rule: {u32 resource, i32 strategy, u32 app_off, u32 app_cnt}: 16 bytes. */
    static final StructLayout AUTHORITY_RULE = MemoryLayout.structLayout(
            JAVA_INT.withName("resource"), JAVA_INT.withName("strategy"),
            JAVA_INT.withName("app_off"), JAVA_INT.withName("app_cnt"));
    private static final long O_RESOURCE = SentinelFlowNative.off(AUTHORITY_RULE, "resource");
    private static final long O_STRATEGY = SentinelFlowNative.off(AUTHORITY_RULE, "strategy");
    private static final long O_APP_OFF = SentinelFlowNative.off(AUTHORITY_RULE, "app_off");
    private static final long O_APP_CNT = SentinelFlowNative.off(AUTHORITY_RULE, "app_cnt");

    /** Loads {@code rules} (null or empty: clears the map); returns the number of rules the engine kept. */
    static int load(MemorySegment engine, List<AuthorityRule> rules, ToIntFunction<String> resourceId,
                    ToIntFunction<String> originId) {
        final int n = rules == null ? 0 : rules.size();
        final List<Integer> apps = new ArrayList<>();
        try (Arena a = Arena.ofConfined()) {
            final long stride = AUTHORITY_RULE.byteSize();
            final MemorySegment table = a.allocate(Math.max(1, n) * stride, 8);
            for (int k = 0; k < n; k++) {
                final AuthorityRule r = rules.get(k);
                final long base = k * stride;
                final boolean blankRes = r == null || StringUtil.isBlank(r.getResource());
                table.set(JAVA_INT, base + O_RESOURCE, blankRes ? -1 : resourceId.applyAsInt(r.getResource()));
                table.set(JAVA_INT, base + O_STRATEGY, r == null ? -1 : r.getStrategy());
                table.set(JAVA_INT, base + O_APP_OFF, apps.size());
                int cnt = 0;
                if (r != null && StringUtil.isNotBlank(r.getLimitApp())) {
                    for (String app : r.getLimitApp().split(",")) {
                        apps.add(originId.applyAsInt(app));
                        cnt++;
                    }
                    if (cnt == 0) {                 // only commas: a valid rule whose list matches no origin
                        apps.add(-1);
                        cnt = 1;
                    }
                }
                table.set(JAVA_INT, base + O_APP_CNT, cnt);
            }
            final MemorySegment ids = a.allocate(Math.max(1, apps.size()) * 4L, 4);
            for (int i = 0; i < apps.size(); i++) ids.setAtIndex(JAVA_INT, i, apps.get(i));
            final MemorySegment kept = a.allocate(4, 4);
            SentinelFlowNative.check((int) SentinelFlowNative.LOAD_AUTHORITY.invokeExact(engine, table, n, ids,
                    apps.size(), kept));
            return kept.get(JAVA_INT, 0);
        } catch (RuntimeException | Error e) {
            throw e;
        } catch (Throwable t) {
            throw new IllegalStateException(t);
        }
    }

    private AuthorityRuleTable() {}
}
