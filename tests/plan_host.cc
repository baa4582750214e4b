// Host-only check of the bucket plan (supernova_amd/csrc/snk_plan.h): built from snk_plan.hip and snk_opts.hip with the host
// compiler, no HIP, and run by tests/test_bucket_plan_host.py.  The expected values follow from the rule as snk_plan.hip documents it,
// each with its arithmetic; none is a measurement.  The geometry is the count kernel's: 2048 table slots, 768 threads, so
// 2048 - 768 - 64 = 1216 usable slots with the margin kernel, 2048 - 2048 / 16 = 1920 booked, 1024 - 64 = 960 behind the bit filter.
#include <stdio.h>
#include <string.h>

#include <initializer_list>

#include "snk_plan.h"

static int failed = 0;
#define CHECK(cond) do { if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); failed = 1; } } while (0)
#define CHECK_EQ(a, b) do { const unsigned long long a_ = (a), b_ = (b); if (a_ != b_) { printf("FAILED line %d: %s = %llu, expected %llu\n", __LINE__, #a, a_, b_); failed = 1; } } while (0)

static snk_opts opts_of(const char* text) {
    snk_opts o;
    snk_opts_init(&o);
    char bad[96];
    if (snk_opts_parse(&o, text, bad, sizeof bad)) { printf("FAILED: option text '%s' (%s)\n", text, bad); failed = 1; }
    return o;
}

// the three callers' parameter sets (the table in snk_plan.h): what they fill besides the job's own figures
static snk_plan_in common(uint32_t K, const snk_opts* o) {
    snk_plan_in in;
    in.K = K; in.min_freq = 3; in.min_bc = 2; in.has_bc = true; in.opts = o;
    in.slots = 2048; in.plain_limit = 1216; in.screen_limit = 960;
    return in;
}
static snk_plan_in resident(uint32_t K, const snk_opts* o) { snk_plan_in in = common(K, o); in.may_adapt = true; in.nb_max = 1ull << 25; in.use_retain = true; return in; }
static snk_plan_in streamed(uint32_t K, const snk_opts* o) { snk_plan_in in = common(K, o); in.may_adapt = true; in.nb_max = 1ull << 23; in.may_book = false; in.fill_unclamped = true; return in; }
static snk_plan_in sharded(uint32_t K, const snk_opts* o, uint32_t world) {
    snk_plan_in in = common(K, o);
    in.may_adapt = true; in.world = world; in.nb_max = 1ull << 26; in.book_only_adapting = true; in.screen_needs_tight = true;
    return in;
}

static const uint64_t BENCH_INST = 100000000ull * (150 - 48 + 1);       // 100 M reads x 103 instances = 1.03e10
static const uint32_t TRIES = 48u << 16;                                // tight_tries' default in the high half

static void derived() {
    const snk_opts none = opts_of("");
    {   // the bench operating point, no hint: 5000 instances per bucket, ceil(1.03e10 / 5000) = 2 060 000
        snk_plan_in in = resident(48, &none);
        in.inst_ub = BENCH_INST;
        snk_plan_out p = snk_bucket_plan(in);
        CHECK_EQ(p.target, 5000); CHECK_EQ(p.NB, 2060000); CHECK_EQ(p.tight, 0); CHECK_EQ(p.screen, 0); CHECK_EQ(p.count_limit, 1216);
        // K = 60: 3500 per bucket, ceil(1.03e10 / 3500) = ceil(2942857.14) = 2 942 858; with K = 60's own 91 instances per read 9.1e9 / 3500 = 2 600 000
        in.K = 60;
        p = snk_bucket_plan(in);
        CHECK_EQ(p.target, 3500); CHECK_EQ(p.NB, 2942858); CHECK_EQ(p.count_limit, 1216);
        in.inst_ub = 100000000ull * 91;
        CHECK_EQ(snk_bucket_plan(in).NB, 2600000);
        // the streamed and the sharded caller reach the same count there
        snk_plan_in t = streamed(48, &none), s = sharded(48, &none, 1);
        t.inst_ub = s.inst_ub = BENCH_INST;
        CHECK_EQ(snk_bucket_plan(t).NB, 2060000); CHECK_EQ(snk_bucket_plan(s).NB, 2060000);
    }
    {   // a forced target: 1.03e10 / 4000 = 2 575 000; the ratio is not asked any more
        const snk_opts o = opts_of("target_inst=4000");
        snk_plan_in in = resident(48, &o);
        in.inst_ub = BENCH_INST; in.may_adapt = false; in.ratio = 0.1;
        snk_plan_out p = snk_bucket_plan(in);
        CHECK_EQ(p.target, 4000); CHECK_EQ(p.NB, 2575000);
    }
    {   // a forced bucket count below the floor: 1.03e10 >> 20 = 9822, + 1 = 9823; above it, it is taken as it is
        snk_plan_in in = resident(48, &none);
        in.inst_ub = BENCH_INST; in.n_buckets = 100; in.may_adapt = false;
        snk_plan_out p = snk_bucket_plan(in);
        CHECK_EQ(p.NB, 9823); CHECK_EQ(p.target, 0);
        in.n_buckets = 12345;
        CHECK_EQ(snk_bucket_plan(in).NB, 12345);
    }
    {   // ranks: 2 060 000 = 8 x 257 500 stays; 3 ranks: ceil(2060000 / 3) = 686 667, x 3 = 2 060 001; a forced count is rounded too: 9823 -> 9824 = 8 x 1228
        snk_plan_in in = sharded(48, &none, 8);
        in.inst_ub = BENCH_INST;
        CHECK_EQ(snk_bucket_plan(in).NB, 2060000);
        in.world = 3;
        CHECK_EQ(snk_bucket_plan(in).NB, 2060001);
        in.world = 8; in.n_buckets = 100;
        CHECK_EQ(snk_bucket_plan(in).NB, 9824);
    }
    {   // tables that run full, ratio 0.5: 0.65 x 1216 / 0.5 = 1580.8 < 5000 -> booked slots, 2048 - 128 = 1920 | 48 << 16.  Without the filter
        // (count_screen_ng = 0) the limit is 1920: 0.65 x 1920 / 0.5 = 2496 < 5000 -> bucket_fill_pct: 0.01 x 50 x 1920 / 0.5 = 1920 per bucket
        const snk_opts o = opts_of("count_screen_ng=0");
        snk_plan_in in = resident(48, &o);
        in.inst_ub = BENCH_INST; in.ratio = 0.5;
        snk_plan_out p = snk_bucket_plan(in);
        CHECK_EQ(p.tight, 1920u | TRIES); CHECK_EQ(p.screen, 0); CHECK_EQ(p.count_limit, 1920); CHECK_EQ(p.target, 1920);
        CHECK_EQ(p.NB, (BENCH_INST + 1919) / 1920);
        // ... the sharded caller takes the same turn
        snk_plan_in s = sharded(48, &o, 2);
        s.inst_ub = BENCH_INST; s.ratio = 0.5;
        snk_plan_out q = snk_bucket_plan(s);
        CHECK_EQ(q.tight, p.tight); CHECK_EQ(q.target, 1920); CHECK_EQ(q.count_limit, 1920);
        // ... the streamed one keeps the default kernel: 0.01 x 50 x 1216 / 0.5 = 1216
        snk_plan_in t = streamed(48, &o);
        t.inst_ub = BENCH_INST; t.ratio = 0.5;
        q = snk_bucket_plan(t);
        CHECK_EQ(q.tight, 0); CHECK_EQ(q.target, 1216); CHECK_EQ(q.count_limit, 1216);
        // the 600 floor: bucket_fill_pct = 25, ratio 1: 0.25 x 1920 / 1 = 480 -> 600
        const snk_opts o25 = opts_of("count_screen_ng=0,bucket_fill_pct=25");
        in.opts = &o25; in.ratio = 1.0;
        CHECK_EQ(snk_bucket_plan(in).target, 600);
        // a ratio that leaves the tables under 65 %: 0.65 x 1216 / 0.1 = 7904 >= 5000 -> the default kernel and size
        in.ratio = 0.1;
        p = snk_bucket_plan(in);
        CHECK_EQ(p.tight, 0); CHECK_EQ(p.target, 5000);
        // a caller that may not adapt still chooses the kernel from the hint, and keeps the default size (resident only)
        in.ratio = 0.5; in.may_adapt = false;
        p = snk_bucket_plan(in);
        CHECK_EQ(p.tight, 1920u | TRIES); CHECK_EQ(p.target, 5000);
        s.may_adapt = false;
        q = snk_bucket_plan(s);
        CHECK_EQ(q.tight, 0); CHECK_EQ(q.target, 5000);
    }
    {   // the bit filter around screen_ratio_pct = 30: off at 0.29, on at 0.31 (level 3, booked slots, 960 usable, screen_target = 4000 per bucket)
        snk_plan_in in = resident(48, &none);
        in.inst_ub = BENCH_INST; in.ratio = 0.29;
        snk_plan_out p = snk_bucket_plan(in);
        CHECK_EQ(p.screen, 0); CHECK_EQ(p.tight, 1920u | TRIES);            // (0.65 x 1216 / 0.29 = 2725 < 5000: booked all the same)
        CHECK_EQ(p.target, 3310);                                           // 0.65 x 1920 / 0.29 = 4303 < 5000 -> 0.5 x 1920 / 0.29 = 3310.3
        in.ratio = 0.31;
        p = snk_bucket_plan(in);
        CHECK_EQ(p.screen, 3); CHECK_EQ(p.tight, 1920u | TRIES); CHECK_EQ(p.count_limit, 960); CHECK_EQ(p.target, 4000); CHECK_EQ(p.NB, 2575000);
        const snk_opts ng0 = opts_of("count_screen_ng=0"), ng2 = opts_of("count_screen_ng=2");
        in.opts = &ng0;
        CHECK_EQ(snk_bucket_plan(in).screen, 0);
        // = 2: always, without any ratio -- the filter brings booked slots with it (resident); the sharded caller wants the ratio to have booked first
        in.opts = &ng2; in.ratio = 0.0;
        p = snk_bucket_plan(in);
        CHECK_EQ(p.screen, 3); CHECK_EQ(p.tight, 1920u | TRIES); CHECK_EQ(p.count_limit, 960); CHECK_EQ(p.target, 4000);
        snk_plan_in s = sharded(48, &ng2, 2);
        s.inst_ub = BENCH_INST;
        CHECK_EQ(snk_bucket_plan(s).screen, 0); CHECK_EQ(snk_bucket_plan(s).tight, 0);
        s.ratio = 0.2;               // 0.65 x 1216 / 0.2 = 3952 < 5000: booked, then the filter
        CHECK_EQ(snk_bucket_plan(s).screen, 3); CHECK_EQ(snk_bucket_plan(s).count_limit, 960);
        // not at K = 60, not below min_freq 3, not with a barcode rule above 2, never in a streamed job
        in.K = 60; CHECK_EQ(snk_bucket_plan(in).screen, 0); in.K = 48;
        in.min_freq = 2; CHECK_EQ(snk_bucket_plan(in).screen, 0); in.min_freq = 3;
        in.min_bc = 3; CHECK_EQ(snk_bucket_plan(in).screen, 0); in.has_bc = false; CHECK_EQ(snk_bucket_plan(in).screen, 3); in.has_bc = true; in.min_bc = 2;
        snk_plan_in t = streamed(48, &ng2);
        t.inst_ub = BENCH_INST; t.ratio = 0.5;
        CHECK_EQ(snk_bucket_plan(t).screen, 0);
        // count_tight = 0 switches the filter off with the booked slots
        const snk_opts off = opts_of("count_screen_ng=2,count_tight=0");
        in.opts = &off; in.ratio = 0.5;
        p = snk_bucket_plan(in);
        CHECK_EQ(p.screen, 0); CHECK_EQ(p.tight, 0); CHECK_EQ(p.count_limit, 1216); CHECK_EQ(p.target, 1216);        // 0.5 x 1216 / 0.5
        // count_tight = n: that many usable slots, at most slots - 64
        const snk_opts t1984 = opts_of("count_tight=1984,count_screen_ng=0,tight_tries=4");
        in.opts = &t1984; in.ratio = 0.0;
        p = snk_bucket_plan(in);
        CHECK_EQ(p.tight, 1984u | (4u << 16)); CHECK_EQ(p.count_limit, 1984); CHECK_EQ(p.target, 5000);
    }
    {   // per-barcode groups: booked slots always; without their filter 0.74 x 1920 = 1420.8 -> 1420 per bucket, limit 1920
        const snk_opts gs0 = opts_of("count_screen=0");
        snk_plan_in in = resident(48, &gs0);
        in.grouped = true; in.has_bc = false; in.min_bc = 0; in.may_adapt = false; in.inst_ub = BENCH_INST;
        snk_plan_out p = snk_bucket_plan(in);
        CHECK_EQ(p.tight, 1920u | TRIES); CHECK_EQ(p.screen, 0); CHECK_EQ(p.target, 1420); CHECK_EQ(p.count_limit, 1920);
        // with it (count_screen = 1 needs min_freq >= 3, = 2 min_freq >= 2): 5200 per bucket, 960 usable slots
        in.opts = &none;
        p = snk_bucket_plan(in);
        CHECK_EQ(p.target, 5200); CHECK_EQ(p.count_limit, 960); CHECK_EQ(p.NB, (BENCH_INST + 5199) / 5200);
        in.min_freq = 2;
        CHECK_EQ(snk_bucket_plan(in).target, 1420);
        const snk_opts gs2 = opts_of("count_screen=2");
        in.opts = &gs2;
        CHECK_EQ(snk_bucket_plan(in).target, 5200);
        // count_tight = 0: the margin kernel, 0.74 x 1216 = 899.84 -> 899
        const snk_opts off = opts_of("count_tight=0");
        in.opts = &off; in.min_freq = 3;
        p = snk_bucket_plan(in);
        CHECK_EQ(p.tight, 0); CHECK_EQ(p.target, 899); CHECK_EQ(p.count_limit, 1216);
    }
    {   // the retained-share rule: chunk_kmers 180 / 0.1 retained per instance = 1800 < 5000 -> 1800 per bucket
        const snk_opts o = opts_of("count_screen_ng=0");
        snk_plan_in in = resident(48, &o);
        in.inst_ub = BENCH_INST; in.retain = 0.1;
        CHECK_EQ(snk_bucket_plan(in).target, 1800);
        // with a ratio of 0.5 the fill rule says 1920 (above): the tighter of the two is 1800; at bucket_fill_pct = 25 it says 0.25 x 1920 / 0.5 = 960
        in.ratio = 0.5;
        CHECK_EQ(snk_bucket_plan(in).target, 1800);
        const snk_opts o25 = opts_of("count_screen_ng=0,bucket_fill_pct=25");
        in.opts = &o25;
        CHECK_EQ(snk_bucket_plan(in).target, 960);
        // 180 / 0.01 = 18000 >= 5000: the rule does not decide; 180 / 0.5 = 360 -> the 600 floor; the other callers do not use it
        in.opts = &o; in.ratio = 0.0; in.retain = 0.01;
        CHECK_EQ(snk_bucket_plan(in).target, 5000);
        in.retain = 0.5;
        CHECK_EQ(snk_bucket_plan(in).target, 600);
        in.use_retain = false;
        CHECK_EQ(snk_bucket_plan(in).target, 5000);
    }
    {   // the caps: 2^40 instances at 5000 per bucket are 2.2e8 buckets -> nb_max of the caller
        snk_plan_in r = resident(48, &none), t = streamed(48, &none), s = sharded(48, &none, 1);
        r.inst_ub = t.inst_ub = s.inst_ub = 1ull << 40;
        CHECK_EQ(snk_bucket_plan(r).NB, 1u << 25); CHECK_EQ(snk_bucket_plan(t).NB, 1u << 23); CHECK_EQ(snk_bucket_plan(s).NB, 1u << 26);
        // the streamed caller does not cut the fill target at the default: bucket_fill_pct = 100, ratio 0.2: 0.65 x 1216 / 0.2 = 3952 < 5000 and
        // 1216 / 0.2 = 6080 per bucket; the same inputs cut at 5000 elsewhere
        const snk_opts o = opts_of("bucket_fill_pct=100,count_tight=0");
        t.opts = &o; t.ratio = 0.2; r.opts = &o; r.ratio = 0.2;
        CHECK_EQ(snk_bucket_plan(t).target, 6080); CHECK_EQ(snk_bucket_plan(r).target, 5000);
    }
    {   // the history: found again under the same key and read count only
        snk_sizing_history H;
        CHECK(!H.lookup(snk_sizing_key(48, false, 16), 0) || H.ratio == 0.0);
        H.screen_ratio = 0.4;
        H.store(snk_sizing_key(48, false, 16), 20000, 0.25, 0.05);
        CHECK_EQ(snk_sizing_key(48, false, 16), 48 * 2 + 256 * 16); CHECK_EQ(snk_sizing_key(48, true, 20), 48 * 2 + 1 + 256 * 20);
        CHECK(H.lookup(snk_sizing_key(48, false, 16), 20000) && H.ratio == 0.25 && H.retain == 0.05 && H.screen_ratio == 0.4);
        CHECK(!H.lookup(snk_sizing_key(48, true, 16), 20000) && !H.lookup(snk_sizing_key(60, false, 16), 20000) && !H.lookup(snk_sizing_key(48, false, 20), 20000));
        CHECK(!H.lookup(snk_sizing_key(48, false, 16), 20001));
    }
}

// invariants over a grid: K x world x caller x instances x ratio x retained share x option sets at their range ends
static unsigned long long grid() {
    static const char* const OPTS[] = {
        "", "count_tight=0", "count_tight=256", "count_tight=1984,tight_tries=65535", "count_screen_ng=0", "count_screen_ng=2", "count_screen=0", "count_screen=2",
        "screen_ratio_pct=0", "screen_ratio_pct=100", "screen_target=100", "screen_target=1048576", "target_inst=100", "target_inst=1048576", "bucket_fill_pct=1",
        "bucket_fill_pct=100", "adaptive_buckets=0", "chunk_kmers=1", "chunk_kmers=65536", "tight_tries=1",
    };
    const uint64_t INST[] = {0, 1, 103, 2060000, (1ull << 20) - 1, 1ull << 20, BENCH_INST, 1ull << 33, (1ull << 40) - 1, 1ull << 40};
    const double RATIO[] = {0.0, 1e-12, 0.01, 0.158, 0.21, 0.3, 0.41, 1.0};
    const double RETAIN[] = {0.0, 1e-9, 0.05, 1.0};
    const uint32_t WORLD[] = {1, 2, 3, 8}, FORCED[] = {0, 1, 997};
    unsigned long long n = 0;
    for (const char* text : OPTS) {
        const snk_opts o = opts_of(text);
        for (uint32_t K : {48u, 60u}) for (uint32_t world : WORLD) for (int caller = 0; caller < 4; ++caller) for (uint64_t inst : INST) for (double ratio : RATIO)
        for (double retain : RETAIN) for (uint32_t forced : FORCED) {
            if (caller < 2 && world != 1) continue;                    // (one rank off the sharded path)
            if ((retain != 0.0 && caller != 0) || (forced == 1 && ratio != 0.0 && ratio != 0.41)) continue;
            snk_plan_in in = caller == 0 ? resident(K, &o) : caller == 1 ? streamed(K, &o) : sharded(K, &o, world);
            if (caller == 3) { in = resident(48, &o); in.grouped = true; in.has_bc = false; in.min_bc = 0; in.world = world; }      // (groups: K = 48 only)
            in.inst_ub = inst; in.ratio = ratio; in.retain = retain; in.n_buckets = forced;
            in.may_adapt = forced == 0 && !snk_opts_is_set(o, SNK_OPT_target_inst) && caller != 3 && snk_opts_u32(o, SNK_OPT_adaptive_buckets) != 0;
            const snk_plan_out p = snk_bucket_plan(in), again = snk_bucket_plan(in);
            const uint64_t floor_ = (inst >> 20) + 1, up = (in.nb_max + world - 1) / world * world, floor_up = (floor_ + world - 1) / world * world;
            const bool ok = p.NB >= floor_ && p.NB <= (forced ? (forced > floor_up ? (forced + world - 1) / world * world : floor_up) : (up > floor_up ? up : floor_up)) && p.NB % world == 0 &&
                            p.count_limit <= in.slots - 64 && p.count_limit >= 256 && (!p.screen || p.tight != 0) && (forced ? p.target == 0 : (p.target >= 100 && p.target <= 1048576)) &&
                            memcmp(&p, &again, sizeof p) == 0;
            if (!ok) { printf("FAILED grid: opts '%s' K %u world %u caller %d inst %llu ratio %g retain %g forced %u -> NB %u tight %#x screen %u limit %u target %u\n", text, K, world, caller,
                              (unsigned long long)inst, ratio, retain, forced, p.NB, p.tight, p.screen, p.count_limit, p.target); failed = 1; }
            ++n;
        }
    }
    return n;
}

int main() {
    derived();
    const unsigned long long n = grid();
    if (!failed) printf("ok %llu\n", n);
    return failed;
}
