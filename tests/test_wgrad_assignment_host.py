"""The workgroup -> (slice, tile) map of k_mlp_wgrad (csrc/wgrad_assign.hpp), checked on the host: no GPU.

The header is plain C++, so a stand-alone program with its own ``main`` includes it and walks every workgroup count from 1
to 600 (and, for the (tiles, slices) shapes below, the split of an entry into slice and tile that the kernel makes):

  * the map is a bijection onto the slice-major list of (slice, tile) pairs;
  * the workgroups of one ``id % 8`` group (one XCD) receive one contiguous run of that list, in the order of their ids;
  * the runs' lengths are the groups' sizes n_x = (n_wg - x + 7) / 8, and the runs follow each other in group order;
  * fewer than 8 workgroups give the identity.

The program is built with the address and undefined-behaviour sanitizers when the host compiler has them (it is the only
place where a sanitizer can see this code: the kernel itself runs the same three integer expressions)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "deepctr-torch_amd", "csrc")

PROGRAM = r"""
#include <cstdio>
#include <vector>
#include "wgrad_assign.hpp"

static int fail(const char* what, int n_wg, int a, int b) {
  std::printf("FAIL %s: n_wg=%d (%d, %d)\n", what, n_wg, a, b);
  return 1;
}

int main() {
  using namespace dctr;
  for (int n_wg = 1; n_wg <= 600; ++n_wg) {
    std::vector<int> seen(n_wg, 0);
    int start = 0;
    for (int x = 0; x < kXcds; ++x) {
      const int n_x = (n_wg - x + 7) / 8;
      if (wgrad_group_size(n_wg, x) != n_x) return fail("group size", n_wg, x, wgrad_group_size(n_wg, x));
      if (wgrad_group_start(n_wg, x) != start) return fail("group start", n_wg, x, wgrad_group_start(n_wg, x));
      int count = 0;
      for (int wg = x; wg < n_wg; wg += kXcds, ++count) {
        const int e = wgrad_assign(wg, n_wg);
        if (e < 0 || e >= n_wg) return fail("entry out of range", n_wg, wg, e);
        if (e != start + count) return fail("run not contiguous", n_wg, wg, e);
        ++seen[e];
      }
      if (count != n_x) return fail("run length", n_wg, x, count);
      start += n_x;
    }
    if (start != n_wg) return fail("runs do not cover the list", n_wg, start, 0);
    for (int e = 0; e < n_wg; ++e)
      if (seen[e] != 1) return fail("not a bijection", n_wg, e, seen[e]);
    if (n_wg < kXcds)
      for (int wg = 0; wg < n_wg; ++wg)
        if (wgrad_assign(wg, n_wg) != wg) return fail("identity below 8", n_wg, wg, wgrad_assign(wg, n_wg));
  }
  // the kernel's split of an entry: slice = e / n_tiles, tile = e % n_tiles -- every (slice, tile) once, and one group's
  // workgroups on at most two neighbouring slices once a slice has a group's worth of tiles
  const int shapes[][2] = {{1, 1}, {1, 7}, {36, 7}, {12, 16}, {12, 13}, {12, 15}, {6, 16}, {3, 5}, {37, 16}, {5, 1}};
  for (const auto& sh : shapes) {
    const int n_tiles = sh[0], S = sh[1], n_wg = n_tiles * S;
    std::vector<int> pair(n_wg, 0);
    for (int x = 0; x < kXcds; ++x) {
      int lo = S, hi = -1;
      for (int wg = x; wg < n_wg; wg += kXcds) {
        const int e = wgrad_assign(wg, n_wg), s = e / n_tiles, t = e % n_tiles;
        if (s < 0 || s >= S || t < 0 || t >= n_tiles) return fail("pair out of range", n_wg, s, t);
        ++pair[s * n_tiles + t];
        lo = s < lo ? s : lo;
        hi = s > hi ? s : hi;
      }
      if (n_tiles >= wgrad_group_size(n_wg, x) && hi - lo > 1) return fail("more than two slices on a group", n_wg, lo, hi);
    }
    for (int i = 0; i < n_wg; ++i)
      if (pair[i] != 1) return fail("pair not taken once", n_wg, i, pair[i]);
  }
  std::printf("OK\n");
  return 0;
}
"""


def _compiler():
    for c in (os.environ.get("CXX"), "g++", "clang++", "/opt/rocm/bin/hipcc", "hipcc"):
        if c and shutil.which(c):
            return shutil.which(c)
    return None


def test_wgrad_assignment_is_a_grouped_bijection(tmp_path):
    cxx = _compiler()
    assert cxx, "no host C++ compiler (g++, clang++ or hipcc)"
    src = tmp_path / "wgrad_assign_check.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "wgrad_assign_check"
    base = [cxx, "-std=c++17", "-O1", "-g", "-I", CSRC, str(src), "-o", str(exe)]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    # the plain build only where the compiler cannot link ANY program with the sanitizers (no runtimes installed); where it
    # can, a failure of the sanitizer build of this program is a failure of the test
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    have_san = subprocess.run([cxx, "-std=c++17"] + san + [str(probe), "-o", str(tmp_path / "probe")],
                              capture_output=True, text=True).returncode == 0
    print("host check built %s the address and undefined-behaviour sanitizers (%s)" % ("with" if have_san else "WITHOUT", cxx))
    built = subprocess.run(base + (san if have_san else []), capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stdout.strip().endswith("OK"), run.stdout + run.stderr
