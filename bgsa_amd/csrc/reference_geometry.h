// reference_geometry.h — the windows of a mapped reference, as reference_windows.hip, seed_map.hip and pair_map.hip share them
// (include/bgsa_hip.h "a reference as the query set"): L mapped bytes, 1 <= S <= W <= L, n_windows = 1 + ceil((L - W) / S),
// start(w) = min(w * S, L - W).  Internal, not installed.
#pragma once

#include "bgsa_common.h"

namespace bgsa {

// An unnamed namespace, on purpose: Geometry is a kernel argument, and the kernels' names carry its namespace as they did when
// every file had its own struct.  So every including file has its OWN Geometry, window_start and make_geometry: never include
// this header in two files that hand a Geometry to each other.
namespace {

struct Geometry {
    int64_t ref_len, n_windows, last_start;   // last_start = L - W, where the last window is anchored
    int window_len, stride;
};

__host__ __device__ inline int64_t window_start(const Geometry &g, int64_t w)
{
    const int64_t at = w * g.stride;
    return at < g.last_start ? at : g.last_start;
}

// The shape's own checks, in the order every entry point refuses them.  0, or BGSA_HIP_EINVAL with the error text set.
// wide_stride: reference_windows.hip says more about a stride beyond the window.
inline int make_geometry(const char *who, int64_t ref_len, int window_len, int stride, Geometry *out,
                         const char *wide_stride = "the stride exceeds the window length")
{
    if (ref_len < 1) return refuse(who, BGSA_HIP_EINVAL, "ref_len is not positive");
    if (stride < 1) return refuse(who, BGSA_HIP_EINVAL, "the stride is below 1");
    if (stride > window_len) return refuse(who, BGSA_HIP_EINVAL, wide_stride);
    if (window_len > ref_len) return refuse(who, BGSA_HIP_EINVAL, "the window is longer than the reference");
    const int64_t rest = ref_len - window_len;
    *out = Geometry{ref_len, 1 + (rest + stride - 1) / stride, rest, window_len, stride};
    return BGSA_HIP_OK;
}

}  // namespace

}  // namespace bgsa
