// Error plumbing + version for libunigen_hip.so.
#include "ug_common.h"
#include <stdarg.h>

static thread_local char g_err[512] = "";

void ug_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

int ug_check_views(const char* who, const ug_view_rule* rules, int n) {
    for (int i = 0; i < n; ++i) {
        const ug_view_rule& r = rules[i];
        // mult and align are powers of two: masks, not the divisions a run-time divisor would cost on every launch
        UG_REQUIRE(((r.v.rs | r.v.bs) & (r.mult - 1)) == 0 && (reinterpret_cast<uintptr_t>(r.v.p) & (uintptr_t)(r.align - 1)) == 0, UG_ERR_BAD_ALIGN,
                   "%s: %s: strides must be multiples of %d elements and the base %d-byte aligned", who, r.name, r.mult, r.align);
    }
    for (int i = 0; i < n; ++i) {
        const ug_view_rule& r = rules[i];
        UG_REQUIRE(!r.bounded || (r.v.rs > 0 && r.v.rs < (1 << 24)), UG_ERR_UNSUPPORTED,
                   "%s: row strides must be within (0, 2^24) elements: %s has %lld", who, r.name, (long long)r.v.rs);
    }
    return UG_OK;
}

#include <stdlib.h>
#include <string.h>
#include <map>
#include <mutex>
#include <string>

int ug_env_int(const char* name, int dflt) {
    static std::mutex mu;
    static std::map<std::string, int> cache;
    static int dynamic = -1;
    std::lock_guard<std::mutex> lk(mu);
    if (dynamic < 0) { const char* d = getenv("UG_ENV_DYNAMIC"); dynamic = (d && atoi(d) != 0) ? 1 : 0; }
    if (!dynamic) {
        auto it = cache.find(name);
        if (it != cache.end()) return it->second;
    }
    const char* e = getenv(name);
    const int v = (e && *e) ? atoi(e) : dflt;
    cache[name] = v;
    return v;
}

extern "C" const char* ug_last_error(void) { return g_err; }
extern "C" int ug_version(void) { return 240; /* 0.2.4: ug_flash_attn_fwd_wide, flash attention at head width 512 for the AutoencoderKL mid-block (csrc/attn_wide.hip) */ }
