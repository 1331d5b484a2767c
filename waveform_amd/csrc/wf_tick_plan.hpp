// wf_tick_plan.hpp -- the decisions of wf_hip_create that need no device: which transform family an fft size takes
// (plan_transform) and on how many lanes a batch is ticked (plan_lanes).  Plain C++: neither HIP nor the handle is seen here, so
// the decisions can be exercised without a GPU (tests/test_tick_plan_cpu.py).  wf_hip_plan.hip asks once; wf_tick_geom.hip and
// wf_big_dispatch.hip map the finished plan to a kernel instantiation.
#pragma once
#include <cstdint>

#include "wf_config.h"

namespace wf {

enum class Family {
    POW2,           // spectrum_tick_kernel on the geometry of the size itself (512 ... 32768)
    ZERO_PADDED,    // 128 / 256 on the 512-sample geometry (spectrum_tick_kernel<.., DEC>)
    MIXED_RADIX,    // n/2 points as mixed-radix passes inside the Bluestein instantiation of the container (wf_mixed.hpp)
    FIXED_PLAN,     // ... a plan the kernel carries as compile-time constants (plan_id: spectrum_tick_kernel's PLAN)
    BLUESTEIN,      // chirp-z over the container of geom_n / 2 complex points
    WHOLE_65536,    // fft_size 65536: both rows and the end of the tick in one kernel (big_whole_kernel)
    MR_TWO_ROWS,    // above 16384: n/2 as two mixed-radix rows on 512 threads, one kernel (big_mr_whole_kernel)
    MR_ROWS,        // above 16384: big_rows mixed-radix rows, then the epilogue (big_mr_rows_kernel)
    BLUESTEIN_ROWS, // above 16384: big_rows rows, each by Bluestein over br_l points inside LDS (big_br_rows_kernel)
    NONE,           // above 16384 with no row decomposition: no kernel, wf_hip_create refuses (no multiple of 16 ends here)
};

// The development overrides (WF_HIP_* of the environment, read by wf_hip_plan.hip under WF_DEV_BUILD) as plain values; the
// defaults are what the release library does.
struct PlanOverrides {
    int lanes = 0; // WF_HIP_LANES; 0: the rule
};

struct TransformPlan {
    Family family = Family::POW2;
    uint32_t n = 0;        // cfg.fft_size
    uint32_t geom_n = 0;   // the fft size whose geometry runs the batch (big: the row transform's)
    // runs in the Bluestein instantiation of the geometry (BLUESTEIN, MIXED_RADIX, FIXED_PLAN); false for the rows families, which
    // are plain packed real transforms
    bool blu = false;
    // transforms beyond a CU's LDS (wf_big.hpp): big_l complex points per spectrum in big_rows rows
    uint32_t big_l = 0, big_rows = 0;
    uint32_t br_l = 0;     // BLUESTEIN_ROWS: the container length of a row (2048 / 4096 / 8192 complex points)
    uint32_t br_rs = 0;    // ... a row's stride in the scratch buffer: n / 2 / big_rows rounded up to even
    int passes = 0;        // > 0: the mixed-radix passes of the transform (of a row, above 16384)
    int radix[4] = {0, 0, 0, 0};
    bool mr_small = false; // one-wavefront containers: the instantiation that carries the small radices only (<.., MRS>)
    int plan_id = 0;       // FIXED_PLAN: 1 ... 8
    // the channels of a stream run in different workgroups; for mono mixdown also in different launches (TickArgs::split_ch)
    bool want_split = false, split_mono = false;
    float in_scale = 1.0f; // the power of two the window tables carry (wf_hip_internal.hpp)

    bool mr_in_lds() const { return family == Family::MIXED_RADIX || family == Family::FIXED_PLAN; }
    bool big_mr() const { return family == Family::MR_TWO_ROWS || family == Family::MR_ROWS; }
    bool big_mrw() const { return family == Family::MR_TWO_ROWS; }
    bool big_br() const { return family == Family::BLUESTEIN_ROWS; }
    bool big_whole() const { return family == Family::WHOLE_65536; }
};

// `cfg` after wf::normalize_config (and waveform_config / meter_config): a legal fft_size is never refused
TransformPlan plan_transform(const wf_config &cfg, const PlanOverrides &ov); // (no override bears on the transform today)

constexpr int MAX_LANES = 4;
// wg_lds / wg_threads: dynamic LDS and threads of one workgroup of the tick kernel; cu_count: the device's compute units
int plan_lanes(const TransformPlan &t, uint32_t n_streams, uint32_t cap_ch, uint32_t num_bars, uint32_t wg_lds, uint32_t wg_threads,
               int cu_count, const PlanOverrides &ov);

} // namespace wf
