// The tuning switches of a handle (include/snn_amd.h, "Tuning switches"): their fields, and ONE table that says for each its
// name, its value rule, whether snn_set_option and / or the environment (SNN_AMD_<NAME in upper case>, read when the handle is
// created) reach it, and what else a change invalidates.  Plain C++17: tests/cpp/options_table.cpp compiles it alone.
#pragma once
#include <climits>
#include <cstdint>
#include <cstdlib>
#include <string>

namespace snn {

struct Options {      // (what each switch does: include/snn_amd.h, "Tuning switches")
    // on / off
    uint32_t fused_step = 1, dense_close = 0, cells_in_step = 1, update_packs = 1, csr_xcd_bands = 1, csr_image = 1;
    uint32_t resident_quarters = 1, defer_rstdp = 1, uniform_params = 1, stdp_small = 1, halo_peer = 1, verify = 0;
    uint32_t persistent_run = 1;          // (the library clears it itself when a co-residency probe or a run gives up)
    uint32_t persistent_chem = 1, persistent_stdp = 1;
    uint32_t run_timing = 0;              // collect the phase clocks of k_run_resident without printing (snn_get_stat)
    // small ranges
    uint32_t pinned_copies = 1;           // see copy_sync (0: the runtime stages pageable pointers itself)
    uint32_t halo_direct = 1;             // 0 never, 1 snn_run_sharded, 2 also snn_run_sharded_custom
    uint32_t update_all_planes = 1;       // 1 all planes' partials in one thread (default), 2 / 3 the wide update (k_update_wide; measured slower)
    // 0 (default): the scatter kernels right after the step; 1: the update of step t rides on the input pass of step t + 1;
    // 2: prepared delta vectors, applied right away by scatter passes; 3: the row half only (0 wins)
    uint32_t defer_stdp = 0;
    uint32_t stdp_columns_form = 0;       // 0 one thread per presynaptic row, 1 one lane per 16-byte unit (k_stdp_columns_quads)
    uint32_t input_shape = 0;             // 1 | 2: streamed shape of the dense input pass, 0: by size
    // numbers
    uint32_t dense_close_max_chunks = 1u << 30;       // "dense_close" only up to this many chunks of presynaptic rows (experiments)
    uint32_t halo_peer_delay = 0;                     // injected latencies, in s_sleep(127) units (tests)
    uint32_t halo_peer_spin_limit = 1u << 26, run_resident_spin_limit = 1u << 24;      // polls before a waiter gives up (RUN_RESIDENT_SPIN_LIMIT)
    uint32_t run_resident_fault_step = 0;             // test hook, see ResidentRunArgs
    uint32_t run_resident_chunk_steps = 1u << 20;     // test hook: steps per one-launch chunk
    uint32_t verify_fault = 0;            // test hook: word + 1 of the exchange buffer (2^30 + word of the weights) to disturb once
};

// BOOL: v != 0.  RANGE: v if lo <= v <= hi, else the fallback.  CLAMP: min(v, hi) if v >= lo, else the fallback.
// NUMBER: the whole environment string as a decimal number (no option reaches such a row).
enum OptionRule { BOOL, RANGE, CLAMP, NUMBER };
enum OptionSource { OPTION_AND_ENV, OPTION_ONLY, ENV_ONLY };
// what a new value invalidates besides the shadows: the ranks' agreed exchange, the uniform-parameter tables, the probe's verdict
enum OptionAfter { NOTHING, X_AGREED_FALSE, UNI_DIRTY_TRUE, RUN_PROBED_GRID_0 };

struct OptionRow {
    const char *name;
    uint32_t Options::*member;
    OptionRule rule; int lo, hi; uint32_t fallback;
    OptionSource source; OptionAfter after;
};

// The environment path reads the FIRST character only and hands its digit (-1 if it is none) to the same rule as the option:
// SNN_AMD_DEFER_STDP=12 is 1, =x is the fallback 1, SNN_AMD_INPUT_SHAPE=x the fallback 0, SNN_AMD_FUSED_STEP=x (or empty) on.
constexpr OptionRow OPTION_TABLE[] = {
    {"fused_step", &Options::fused_step, BOOL, 0, 1, 0, OPTION_AND_ENV, NOTHING},
    {"dense_close", &Options::dense_close, BOOL, 0, 1, 0, OPTION_AND_ENV, NOTHING},
    {"dense_close_max_chunks", &Options::dense_close_max_chunks, NUMBER, 0, 0, 0, ENV_ONLY, NOTHING},
    {"pinned_copies", &Options::pinned_copies, RANGE, 0, 2, 1, OPTION_AND_ENV, NOTHING},
    {"csr_xcd_bands", &Options::csr_xcd_bands, BOOL, 0, 1, 0, OPTION_AND_ENV, NOTHING},
    {"csr_image", &Options::csr_image, BOOL, 0, 1, 0, OPTION_AND_ENV, NOTHING},
    {"resident_quarters", &Options::resident_quarters, BOOL, 0, 1, 0, OPTION_AND_ENV, NOTHING},
    {"halo_direct", &Options::halo_direct, RANGE, 0, 2, 1, OPTION_AND_ENV, NOTHING},
    {"update_packs", &Options::update_packs, BOOL, 0, 1, 0, OPTION_AND_ENV, NOTHING},
    {"update_all_planes", &Options::update_all_planes, RANGE, 0, 3, 1, OPTION_AND_ENV, NOTHING},
    {"cells_in_step", &Options::cells_in_step, BOOL, 0, 1, 0, OPTION_AND_ENV, NOTHING},
    {"defer_rstdp", &Options::defer_rstdp, BOOL, 0, 1, 0, OPTION_AND_ENV, NOTHING},
    {"defer_stdp", &Options::defer_stdp, RANGE, 0, 3, 1, OPTION_AND_ENV, NOTHING},
    {"uniform_params", &Options::uniform_params, BOOL, 0, 1, 0, OPTION_AND_ENV, UNI_DIRTY_TRUE},
    {"persistent_run", &Options::persistent_run, BOOL, 0, 1, 0, OPTION_AND_ENV, RUN_PROBED_GRID_0},
    {"persistent_chem", &Options::persistent_chem, BOOL, 0, 1, 0, OPTION_AND_ENV, NOTHING},
    {"persistent_stdp", &Options::persistent_stdp, BOOL, 0, 1, 0, OPTION_AND_ENV, NOTHING},
    {"halo_peer", &Options::halo_peer, BOOL, 0, 1, 0, OPTION_AND_ENV, X_AGREED_FALSE},
    {"halo_peer_delay", &Options::halo_peer_delay, CLAMP, 0, 64, 0, OPTION_ONLY, NOTHING},
    {"halo_peer_spin_limit", &Options::halo_peer_spin_limit, CLAMP, 1, INT_MAX, 1u << 26, OPTION_ONLY, NOTHING},
    {"stdp_columns_form", &Options::stdp_columns_form, RANGE, 1, 1, 0, OPTION_AND_ENV, NOTHING},
    {"stdp_small", &Options::stdp_small, BOOL, 0, 1, 0, OPTION_AND_ENV, NOTHING},
    {"input_shape", &Options::input_shape, RANGE, 1, 2, 0, OPTION_AND_ENV, NOTHING},
    {"run_resident_spin_limit", &Options::run_resident_spin_limit, CLAMP, 1, INT_MAX, 1u << 24, OPTION_ONLY, NOTHING},
    {"run_resident_fault_step", &Options::run_resident_fault_step, CLAMP, 0, INT_MAX, 0, OPTION_ONLY, NOTHING},
    {"run_resident_chunk_steps", &Options::run_resident_chunk_steps, CLAMP, 4, 1 << 20, 1u << 20, OPTION_ONLY, NOTHING},
    {"run_timing", &Options::run_timing, BOOL, 0, 1, 0, OPTION_ONLY, NOTHING},
    {"verify", &Options::verify, BOOL, 0, 1, 0, OPTION_AND_ENV, NOTHING},
    {"verify_fault", &Options::verify_fault, CLAMP, 1, INT_MAX, 0, OPTION_ONLY, NOTHING},
};

// the value rule of a row, for snn_set_option's int and (through option_from_env) for the environment
inline uint32_t option_value(const OptionRow &r, int v)
{
    if (r.rule == BOOL) return v != 0;
    if (v < r.lo || (r.rule == RANGE && v > r.hi)) return r.fallback;
    return (uint32_t)(v < r.hi ? v : r.hi);
}
inline uint32_t option_from_env(const OptionRow &r, const char *e)
{
    if (r.rule == NUMBER) return (uint32_t)strtoul(e, nullptr, 10);
    return option_value(r, (e[0] >= '0' && e[0] <= '9') ? e[0] - '0' : -1);
}
inline std::string option_env_name(const OptionRow &r)
{
    std::string s = "SNN_AMD_";
    for (const char *c = r.name; *c; ++c) s += (char)(*c >= 'a' && *c <= 'z' ? *c - 32 : *c);
    return s;
}

} // namespace snn
