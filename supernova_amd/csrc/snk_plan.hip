// snk_plan.hip -- the bucket plan of a count call (snk_plan.h): plain host code, the record of the measurements behind every figure.
#include "snk_plan.h"

#include <algorithm>

// Instances per bucket: sized so that the DISTINCT k-mers of a bucket fit the LDS table (1216 claims).  At 56x coverage and 0.2 % errors
// 5000 instances hold ~800 distinct k-mers; per-barcode groups see every locus once or twice, so nearly every instance is distinct
// there.  Error-rich or shallow data have more distinct k-mers per instance: with the default size nearly every bucket would overflow
// its table and be counted in two to four hash-split sub-passes (0.6 % errors: count 46 -> 133 ms).  The ratio is a property of the data
// set: the previous call's is used if there is one (snk_sizing_history), else the count stage looks at its first 1/64 of the buckets
// and asks for a second partition when they overflow as a rule (the caller's loop, SNK_RETARGET).
snk_plan_out snk_bucket_plan(const snk_plan_in& in) {
    const snk_opts& o = *in.opts;
    snk_plan_out out;
    const uint32_t plain_target = in.K == 48 ? 5000u : 3500u;
    const bool target_forced = snk_opts_is_set(o, SNK_OPT_target_inst);
    const uint32_t tries = snk_opts_u32(o, SNK_OPT_tight_tries) << 16;
    const uint32_t booked = (in.slots - in.slots / 16u) | tries;
    const bool tight_off = snk_opts_is_set(o, SNK_OPT_count_tight) && snk_opts_u32(o, SNK_OPT_count_tight) == 0u;
    auto limit_of = [&](uint32_t tight) -> uint32_t { return tight ? (tight & 0xFFFFu) : in.plain_limit; };      // (snk_count_limit)
    const double rt = in.may_adapt ? in.ratio : 0.0;             // the ratio the bucket target follows ...
    const double rk = (!in.book_only_adapting || (in.n_buckets == 0 && !target_forced && rt > 0.0)) ? in.ratio : 0.0;      // ... and the one the kernel choice sees

    // The count kernel has two ways to keep its probe loops supplied with free slots (snk_count.hip): a margin of one round of every wave
    // (1216 of 2048 slots usable, nothing to pay per round) or booked slots (15/16 usable, one LDS atomic round trip per wave and round:
    // 45.1 instead of 43.0 ms on the bench model).  Data whose tables run full -- sequencing errors, per-barcode groups -- are counted the
    // second way: fewer, fuller buckets (1.5 % errors: 8.4 M -> 5.6 M buckets, 218 -> 188 ms; 0.6 %: 149 -> 136; groups: 183 -> 177).
    // count_tight = 0 never, = n always with n usable slots.
    if (in.may_book) {
        if (snk_opts_is_set(o, SNK_OPT_count_tight) && (tight_off || !in.book_only_adapting)) {
            const uint32_t v = snk_opts_u32(o, SNK_OPT_count_tight);
            out.tight = v ? (std::min(std::max(v, 256u), in.slots - 64u) | tries) : 0u;
        } else if (in.grouped || (rk > 0.0 && 0.65 * (double)in.plain_limit / rk < (double)plain_target))
            out.tight = booked;
    }
    // Ungrouped reads whose tables run very full (1.5 % errors: 0.41 distinct k-mers per instance, most of them seen once or twice): the bit
    // filter of the per-barcode groups in front of a 1024-slot table -- the table then sees what can be retained and the bucket is as large
    // as one batch of records and ten instances per lane allow.  count_screen_ng: 0 never, 2 always, default: ratio above 0.3
    // (0.6 % errors, ratio 0.21, lose with it: a fifth of their instances are singletons, the first pass costs more than it saves).
    // The filter comes with booked slots: count_tight = 0 switches it off too.
    {
        const uint32_t ng = snk_opts_u32(o, SNK_OPT_count_screen_ng);
        const bool allowed = in.may_book && !tight_off && !in.grouped && in.K == 48 && in.min_freq >= 3 && (!in.has_bc || in.min_bc <= 2);
        if (allowed && ng && (ng >= 2 || rk > 0.01 * snk_opts_u32(o, SNK_OPT_screen_ratio_pct)) && (!in.screen_needs_tight || out.tight)) out.screen = 3u;
        if (out.screen && !out.tight) out.tight = booked;
    }
    // (groups behind THEIR bit filter -- option count_screen, min_freq >= 2: the table only sees the (group, k-mer) pairs that can be retained, one in ten)
    const uint32_t gs = snk_opts_u32(o, SNK_OPT_count_screen);
    const bool group_screen = in.grouped && gs != 0 && in.min_freq >= (gs >= 2 ? 2u : 3u);
    out.count_limit = limit_of(out.tight);
    if ((out.screen || (group_screen && out.tight)) && in.K == 48) out.count_limit = std::min(out.count_limit, in.screen_limit);

    uint64_t nb = in.n_buckets;
    if (nb == 0) {
        // per-barcode groups: nearly every instance is a distinct entry, the bucket IS the table: three quarters of its capacity on average
        // ... unless the bit filter is on: then a bucket is as large as one batch of 512 records and ten instances per lane allow: beyond
        // 6000 buckets start to fall out of the filter -- 92.9 ms at 4800, 92.2 at 5600, 94.6 at 6400, `profiles/r05_count_screen_groups.log`
        const uint32_t default_target = in.grouped ? ((group_screen && out.tight) ? 5200u : (uint32_t)(0.74 * limit_of(out.tight))) : plain_target;
        const double lim = (double)limit_of(out.tight);
        // measured: the default size is right while the tables run up to ~65 % full on average (the bench model: 800 of 1216); data
        // that would fill them further do best at ~50 % (0.6 % errors: 239 ms with the default size, 186 at 80 %, 154 at 50 %)
        const bool fuller = rt > 0.0 && 0.65 * lim / rt < (double)default_target;
        const double t_fill = fuller ? 0.01 * snk_opts_u32(o, SNK_OPT_bucket_fill_pct) * lim / rt : 0.0;
        uint32_t target = default_target;
        // ... and the RETAINED k-mers of a bucket are one chunk of the bucket-local graph stage, whose one-wave kernels hold 256 of them
        // (larger chunks take the slower big-chunk variants): at half the coverage twice as many k-mers survive per instance, every other
        // chunk was over the line and the graph stage took 81 instead of ~58 ms.  From the previous call's retained share: chunks of ~180
        // (28x coverage, with merged chunks behind it: 153.2 ms at 120, 149.5 at 150, 147.7 at 180, 147.5 at 210).
        // (groups behind the bit filter: buckets of 5200 instances, unless that many would retain more than a graph chunk holds)
        const double t_chunk = (in.use_retain && in.retain > 0.0 && (!in.grouped || group_screen)) ? (double)snk_opts_u32(o, SNK_OPT_chunk_kmers) / in.retain : 0.0;
        if (target_forced) target = snk_opts_u32(o, SNK_OPT_target_inst);
        else if (out.screen) target = snk_opts_u32(o, SNK_OPT_screen_target);
        else if (t_chunk > 0.0 && t_chunk < (double)default_target) {
            target = t_chunk < 600.0 ? 600u : (uint32_t)t_chunk;
            if (fuller && t_fill < (double)target) target = t_fill < 600.0 ? 600u : (uint32_t)t_fill;           // the tighter of the two limits
        } else if (fuller)
            target = (t_fill >= (double)default_target && !in.fill_unclamped) ? default_target : (t_fill < 600.0 ? 600u : (uint32_t)t_fill);
        nb = (in.inst_ub + target - 1) / target;
        if (nb < 1) nb = 1;
        if (nb > in.nb_max) nb = in.nb_max;
        out.target = target;
    }
    // a caller's bucket count is honoured down to ~1 M k-mer instances per bucket: a bucket is counted by ONE workgroup that re-reads all
    // its records in every hash-split sub-pass, so 20 M instances in one bucket would be thousands of passes over a million records
    // (finite, but minutes)
    const uint64_t nb_floor = (in.inst_ub >> 20) + 1;
    if (nb < nb_floor) nb = nb_floor;
    nb = (nb + in.world - 1) / in.world * in.world;
    out.NB = (uint32_t)nb;
    return out;
}
