// snk_opts.hip -- the option registry behind snk_ctx_set_option / snk_ctx_set_tuning (snk_opts.h).
// With SNK_OPTS_NO_CTX defined this file is the registry alone -- names, defaults, ranges, parsing, the value of an option in a set of
// options: host code without a HIP header or a context, which the host-only checks link (tests/plan_host.cc).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>

#include "snk_opts.h"
#ifndef SNK_OPTS_NO_CTX
#include "snk_ctx.h"
#endif

const snk_opt_def snk_opt_defs[SNK_OPT_COUNT] = {
#define X(name, dflt, range, doc) {#name, dflt, range, doc},
    SNK_OPTIONS(X)
#undef X
};

int snk_opt_index(const char* name) {
    if (!name) return -1;
    for (int i = 0; i < SNK_OPT_COUNT; ++i) if (strcmp(snk_opt_defs[i].name, name) == 0) return i;
    return -1;
}
void snk_opts_init(snk_opts* o) { memset(o, 0, sizeof *o); }

int snk_opts_parse(snk_opts* o, const char* text, char* bad, unsigned badcap) {
    if (!text) return 0;
    const char* p = text;
    while (*p) {
        while (*p == ',' || *p == ' ' || *p == ';') ++p;
        if (!*p) break;
        const char* e = p;
        while (*e && *e != ',' && *e != ';' && *e != ' ') ++e;
        char item[96];
        const size_t n = (size_t)(e - p) < sizeof item - 1 ? (size_t)(e - p) : sizeof item - 1;
        memcpy(item, p, n);
        item[n] = 0;
        char* eq = strchr(item, '=');
        int ix = -1;
        char* endp = nullptr;
        long long v = 0;
        if (eq) { *eq = 0; ix = snk_opt_index(item); v = strtoll(eq + 1, &endp, 0); }
        if (ix < 0 || !eq || endp == eq + 1 || *endp || !snk_opt_valid(ix, v)) {
            if (eq) *eq = '=';
            if (bad && badcap) { strncpy(bad, item, badcap - 1); bad[badcap - 1] = 0; }
            return -1;
        }
        o->v[ix] = v; o->set[ix] = true;
        p = e;
    }
    return 0;
}

// the registry's range of the option (snk_opts.h says where each comes from)
bool snk_opt_valid(int id, long long value) {
    if (id < 0 || id >= SNK_OPT_COUNT) return false;
    const snk_opt_def& d = snk_opt_defs[id];
    return (value == 0 && d.zero) || (value >= d.lo && value <= d.hi && (value - d.lo) % d.step == 0);
}

// "<text> [lo..hi]", "[0 or lo..hi]", "[lo..hi step s]": what snk_option_doc and the setters' refusals show
const char* snk_opt_doc(int id) {
    static const struct docs {
        std::string text[SNK_OPT_COUNT];
        docs() {
            for (int i = 0; i < SNK_OPT_COUNT; ++i) {
                const snk_opt_def& d = snk_opt_defs[i];
                char r[96];
                int n = snprintf(r, sizeof r, " [%s%lld..%lld", d.zero ? "0 or " : "", d.lo, d.hi);
                if (d.step != 1) n += snprintf(r + n, sizeof r - (size_t)n, " step %lld", d.step);
                snprintf(r + n, sizeof r - (size_t)n, "]");
                text[i] = std::string(d.doc) + r;
            }
        }
    } all;
    return id >= 0 && id < SNK_OPT_COUNT ? all.text[id].c_str() : nullptr;
}

bool snk_opts_is_set(const snk_opts& o, snk_opt_id id) { return o.set[id]; }
unsigned long long snk_opts_u64(const snk_opts& o, snk_opt_id id) { return (unsigned long long)(o.set[id] ? o.v[id] : snk_opt_defs[id].dflt); }

#ifndef SNK_OPTS_NO_CTX
bool snk_opt_is_set(const snk_ctx* ctx, snk_opt_id id) { return ctx && snk_opts_is_set(ctx->opts, id); }
uint32_t snk_opt_u32(const snk_ctx* ctx, snk_opt_id id) { return (uint32_t)snk_opt_u64(ctx, id); }
unsigned long long snk_opt_u64(const snk_ctx* ctx, snk_opt_id id) { return ctx ? snk_opts_u64(ctx->opts, id) : (unsigned long long)snk_opt_defs[id].dflt; }

// ---- C ABI
extern "C" int snk_ctx_set_option(snk_ctx* ctx, const char* name, long long value, char* err, size_t errcap) {
    if (!ctx || !name) return snk_fail(SNK_E_ARG, err, errcap, "snk_ctx_set_option: NULL argument");
    const int ix = snk_opt_index(name);
    if (ix < 0) return snk_fail(SNK_E_ARG, err, errcap, "snk_ctx_set_option: no option '%s' (snk_option_name lists them)", name);
    if (!snk_opt_valid(ix, value)) return snk_fail(SNK_E_ARG, err, errcap, "snk_ctx_set_option: %lld is out of range for '%s' (%s)", value, name, snk_opt_doc(ix));
    ctx->opts.v[ix] = value; ctx->opts.set[ix] = true;
    return SNK_OK;
}
extern "C" int snk_option_check(const char* name, long long value, char* err, size_t errcap) {
    const int ix = snk_opt_index(name);
    if (ix < 0) return snk_fail(SNK_E_ARG, err, errcap, "snk_option_check: no option '%s'", name ? name : "(NULL)");
    if (!snk_opt_valid(ix, value)) return snk_fail(SNK_E_ARG, err, errcap, "snk_option_check: %lld is out of range for '%s' (%s)", value, name, snk_opt_doc(ix));
    return SNK_OK;
}
extern "C" int snk_ctx_clear_option(snk_ctx* ctx, const char* name) {
    if (!ctx) return SNK_E_ARG;
    if (!name) { snk_opts_init(&ctx->opts); return SNK_OK; }
    const int ix = snk_opt_index(name);
    if (ix < 0) return SNK_E_ARG;
    ctx->opts.set[ix] = false; ctx->opts.v[ix] = 0;
    return SNK_OK;
}
extern "C" int snk_ctx_get_option(const snk_ctx* ctx, const char* name, long long* value) {
    if (!ctx) return SNK_E_ARG;
    const int ix = snk_opt_index(name);
    if (ix < 0) return SNK_E_ARG;
    if (value) *value = ctx->opts.v[ix];
    return ctx->opts.set[ix] ? 1 : 0;
}
extern "C" const char* snk_option_name(uint32_t i) { return i < (uint32_t)SNK_OPT_COUNT ? snk_opt_defs[i].name : nullptr; }
extern "C" const char* snk_option_doc(uint32_t i) { return i < (uint32_t)SNK_OPT_COUNT ? snk_opt_doc((int)i) : nullptr; }

// the documented knobs as one struct: 0 in a field = the library's own choice (the option is cleared)
namespace {
struct tfield { snk_opt_id opt; size_t off; };
#define TF(f, o) {SNK_OPT_##o, offsetof(snk_tuning, f)}
const tfield tfields[] = {
    TF(count_screen_ratio_pct, screen_ratio_pct), TF(target_inst, target_inst), TF(bucket_fill_pct, bucket_fill_pct),
    TF(minimiser_len, minimiser_len), TF(partition_passes, partition_passes), TF(hot_min, hot_min), TF(hot_factor, hot_factor),
    TF(hot_class_inst, hot_class_inst), TF(exchange_ranges, exchange_ranges), TF(hbv_dev_min, hbv_dev_min), TF(hbv_big, hbv_big),
    TF(chunk_kmers, chunk_kmers), TF(unitig_bc_cut, unitig_bc_cut),
};
#undef TF
}  // namespace

extern "C" void snk_tuning_default(snk_tuning* t) { if (t) memset(t, 0, sizeof *t); }

extern "C" int snk_ctx_set_tuning(snk_ctx* ctx, const snk_tuning* t, char* err, size_t errcap) {
    if (!ctx || !t) return snk_fail(SNK_E_ARG, err, errcap, "snk_ctx_set_tuning: NULL argument");
    if (t->count_kernel > SNK_COUNT_KERNEL_SCREEN) return snk_fail(SNK_E_ARG, err, errcap, "snk_ctx_set_tuning: count_kernel %u", t->count_kernel);
    if (t->path_lookup > 2 || t->join_ranking > 2 || t->adaptive_buckets > 2 || t->hot_buckets > 2)
        return snk_fail(SNK_E_ARG, err, errcap, "snk_ctx_set_tuning: a 0/1/2 field is out of range");
    auto field = [&](const tfield& f) { return *reinterpret_cast<const uint32_t*>(reinterpret_cast<const char*>(t) + f.off); };
    // a field that is not 0 is a value of its option and has that option's range; nothing is applied unless everything is in range
    for (const tfield& f : tfields)
        if (field(f) && !snk_opt_valid(f.opt, field(f)))
            return snk_fail(SNK_E_ARG, err, errcap, "snk_ctx_set_tuning: %u is out of range for '%s' (%s)", field(f), snk_opt_defs[f.opt].name, snk_opt_doc(f.opt));
    const uint32_t slots = t->count_tight_slots ? t->count_tight_slots : 1920u;
    if (t->count_kernel == SNK_COUNT_KERNEL_BOOKED && !snk_opt_valid(SNK_OPT_count_tight, slots))
        return snk_fail(SNK_E_ARG, err, errcap, "snk_ctx_set_tuning: count_tight_slots %u is out of range (%s)", slots, snk_opt_doc(SNK_OPT_count_tight));
    auto put = [&](snk_opt_id o, bool on, long long v) { ctx->opts.set[o] = on; ctx->opts.v[o] = on ? v : 0; };
    for (const tfield& f : tfields) put(f.opt, field(f) != 0, field(f));
    // count kernel: auto | margin (the default kernel) | booked slots | bit filter + booked slots
    switch (t->count_kernel) {
        case SNK_COUNT_KERNEL_AUTO: put(SNK_OPT_count_tight, false, 0); put(SNK_OPT_count_screen_ng, false, 0); break;
        case SNK_COUNT_KERNEL_MARGIN: put(SNK_OPT_count_tight, true, 0); put(SNK_OPT_count_screen_ng, true, 0); break;
        case SNK_COUNT_KERNEL_BOOKED: put(SNK_OPT_count_tight, true, slots); put(SNK_OPT_count_screen_ng, true, 0); break;
        case SNK_COUNT_KERNEL_SCREEN: put(SNK_OPT_count_tight, false, 0); put(SNK_OPT_count_screen_ng, true, 2); break;
    }
    put(SNK_OPT_adaptive_buckets, t->adaptive_buckets != 0, t->adaptive_buckets == 1 ? 1 : 0);       // 1 on, 2 off
    put(SNK_OPT_hot, t->hot_buckets != 0, t->hot_buckets == 1 ? 1 : 0);
    put(SNK_OPT_path_index, t->path_lookup != 0, t->path_lookup == 1 ? 1 : 0);                        // 1 index, 2 dictionary
    put(SNK_OPT_join_replicated, t->join_ranking != 0, t->join_ranking == 2 ? 1 : 0);                 // 1 partitioned, 2 replicated
    return SNK_OK;
}

extern "C" void snk_ctx_get_tuning(const snk_ctx* ctx, snk_tuning* t) {
    if (!ctx || !t) return;
    memset(t, 0, sizeof *t);
    auto get = [&](snk_opt_id o, long long* v) { *v = (long long)snk_opt_u64(ctx, o); return snk_opt_is_set(ctx, o); };
    long long v;
    for (const tfield& f : tfields) if (get(f.opt, &v)) *reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(t) + f.off) = (uint32_t)v;
    long long tight = 0, ng = 0;
    const bool ts = get(SNK_OPT_count_tight, &tight), ns = get(SNK_OPT_count_screen_ng, &ng);
    if (ns && ng >= 2) t->count_kernel = SNK_COUNT_KERNEL_SCREEN;
    else if (ts && tight) { t->count_kernel = SNK_COUNT_KERNEL_BOOKED; t->count_tight_slots = (uint32_t)tight; }
    else if (ts) t->count_kernel = SNK_COUNT_KERNEL_MARGIN;
    if (get(SNK_OPT_adaptive_buckets, &v)) t->adaptive_buckets = v ? 1 : 2;
    if (get(SNK_OPT_hot, &v)) t->hot_buckets = v ? 1 : 2;
    if (get(SNK_OPT_path_index, &v)) t->path_lookup = v ? 1 : 2;
    if (get(SNK_OPT_join_replicated, &v)) t->join_ranking = v ? 2 : 1;
    // what the last call on the context chose
    t->last_count_limit = ctx->last_count_limit;
    t->last_count_kernel = ctx->count_screen ? SNK_COUNT_KERNEL_SCREEN : (ctx->count_tight ? SNK_COUNT_KERNEL_BOOKED : SNK_COUNT_KERNEL_MARGIN);
    t->last_partition_passes = ctx->last_partition_passes;
    t->last_minimiser_len = ctx->mlen;
}
#endif  // SNK_OPTS_NO_CTX
