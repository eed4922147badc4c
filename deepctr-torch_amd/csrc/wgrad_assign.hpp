// wgrad_assign.hpp -- which (batch slice, 64x64 tile) a GEMM workgroup of k_mlp_wgrad computes.
//
// Workgroups are dealt round-robin over the 8 XCDs (workgroup id % 8), each with an L2 of its own.  A slice's operand
// panels (its rows of the layer inputs and of dh, ~2.5 MB at the DeepFM tower) fit one L2, the seven slices together
// (19 MB) fit none: with workgroup -> (tile, slice) in plain order every L2 saw every slice and every tile re-read its two
// panels from beyond L2.  Here the (slice, tile) pairs are listed slice-major, all layers' tiles of slice 0 first, and the
// workgroups of one id % 8 group take one contiguous run of that list, so an XCD works on at most two neighbouring
// slices.  The runs' lengths are the groups' sizes, whatever n_wg is (no divisibility needed; fewer than 8 workgroups give
// the identity).  The map is a bijection: every pair is computed once, with the same instructions, into the same place --
// it is for speed only, nothing may depend on where a workgroup runs.
//
// Plain C++ without includes on purpose: tests/test_wgrad_assignment_host.py compiles it into a host program.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DCTR_HOST_DEVICE __host__ __device__
#else
#define DCTR_HOST_DEVICE
#endif

namespace dctr {

constexpr int kXcds = 8;

// workgroups of group x = id % 8 among n_wg, and the workgroups of the groups before it
DCTR_HOST_DEVICE inline int wgrad_group_size(int n_wg, int x) { return (n_wg - x + kXcds - 1) / kXcds; }
DCTR_HOST_DEVICE inline int wgrad_group_start(int n_wg, int x) {
  const int q = n_wg / kXcds, r = n_wg % kXcds;      // group y has q + (y < r) workgroups
  return x * q + (x < r ? x : r);
}

// GEMM workgroup `wg` of n_wg = n_tiles * S -> its entry of the slice-major list: slice = entry / n_tiles, tile (counted
// through the layers) = entry % n_tiles
DCTR_HOST_DEVICE inline int wgrad_assign(int wg, int n_wg) {
  return wgrad_group_start(n_wg, wg % kXcds) + wg / kXcds;
}

}  // namespace dctr
