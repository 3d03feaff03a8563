"""The host-only core of cnn_graph_amd/csrc/launch.h compiled with g++ against
stand-ins that count their calls: the once-per-(device, kernel) opt-in behind
allow_big_lds, the resident-count cache behind resident_blocks, the per-device
integer behind device_cus, and what the three callers make of an unknown count.

The opt-in used to be a function-local static per call site: set once per
process on whatever device was current at the first launch, so a second device
launched with a function attribute that was never set there."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "cnn_graph_amd", "csrc")

SRC = r"""
#include "launch.h"
#include <chrono>
#include <cstdio>
#include <vector>
static int kern_a, kern_b, kern_c, kern_d;
static std::atomic<int> calls{0};

static void once() {
  cg::OncePerDevice t;
  auto ok = [&] { ++calls; return 0; };
  auto bad = [&] { ++calls; return 719; };
  int sum = 0;
  for (int i = 0; i < 1000; ++i) sum += t.get(0, &kern_a, ok);
  const int one = calls;                       // 1: one kernel, one device, many calls
  sum += t.get(1, &kern_a, ok);
  sum += t.get(1, &kern_a, ok);
  const int dev1 = calls - one;                // 1: the second device's own call
  sum += t.get(0, &kern_b, ok);
  sum += t.get(0, &kern_b, ok);
  const int kern2 = calls - one - dev1;        // 1: the second kernel's own call
  const int before = calls;
  const int f0 = t.get(0, &kern_c, bad), f1 = t.get(0, &kern_c, bad), f2 = t.get(0, &kern_c, ok);
  const int failed_calls = calls - before;     // 1: a failed setter is not called again
  const int other_dev = t.get(1, &kern_c, ok); // 0: the failure belongs to device 0
  // a device the table has no column for: set on every call, never skipped
  const int before_far = calls;
  sum += t.get(cg::OncePerDevice::kDevices, &kern_a, ok) + t.get(-1, &kern_a, ok);
  const int far_calls = calls - before_far;
  printf("once %d %d %d %d %d %d %d %d %d %d\n", sum, one, dev1, kern2, f0, f1, f2, failed_calls,
         other_dev, far_calls);
}

static void threads() {
  // eight threads, one fresh key: one setter call, and nobody returns before
  // the setter has (it sleeps, and `finished` is set as its last act)
  cg::OncePerDevice t;
  std::atomic<int> set_calls{0}, finished{0}, early{0}, wrong{0}, go{0};
  std::vector<std::thread> th;
  for (int i = 0; i < 8; ++i)
    th.emplace_back([&] {
      while (!go.load()) std::this_thread::yield();
      const int st = t.get(3, &kern_d, [&] {
        ++set_calls;
        std::this_thread::sleep_for(std::chrono::milliseconds(20));
        finished.store(1);
        return 7;
      });
      if (!finished.load()) ++early;
      if (st != 7) ++wrong;
    });
  go.store(1);
  for (auto& x : th) x.join();
  printf("threads %d %d %d\n", set_calls.load(), early.load(), wrong.load());
}

// stand-in occupancy: a 160 KB LDS budget per CU, 256 CUs on device 0 and 128
// on device 1; kernel b's query fails
static int queries = 0;
static int resident(cg::ResidentCache& c, int dev, const void* k, int threads, size_t lds) {
  return c.get(dev, k, threads, lds, [&](const void* kf, int, size_t l, int* per_cu, int* cus) {
    ++queries;
    *per_cu = int((160 * 1024) / l);
    *cus = dev == 0 ? 256 : 128;
    return kf != &kern_b;
  });
}

static void counts() {
  cg::ResidentCache c;
  const size_t lds = 80 * 1024;
  int r0 = 0;
  for (int i = 0; i < 5; ++i) r0 = resident(c, 0, &kern_a, 256, lds);
  const int q_one = queries;                                 // 1
  const int r1 = resident(c, 1, &kern_a, 256, lds);          // device
  const int r2 = resident(c, 0, &kern_c, 256, lds);          // kernel
  const int r3 = resident(c, 0, &kern_a, 512, lds);          // threads
  const int r4 = resident(c, 0, &kern_a, 256, 40 * 1024);    // LDS
  const int q_keys = queries;                                // 5
  const int unknown = resident(c, 0, &kern_b, 256, lds);     // the query fails
  (void)resident(c, 0, &kern_b, 256, lds);
  const int q_fail = queries - q_keys;                       // 1: the failure is cached too
  printf("counts %d %d %d %d %d %d %d %d %d\n", r0, q_one, r1, r2, r3, r4, q_keys, unknown, q_fail);
  // the callers' policies on the unknown count and on a known one
  printf("policy %u %u %d %d %d %d %d\n", cg::persistent_grid(5000, unknown, 1),
         cg::persistent_grid(5000, r0, 1), cg::xbasis_resident(unknown), cg::xbasis_resident(r0),
         int(cg::grid_fit(256, unknown)), int(cg::grid_fit(2 * 256 + 2, r0)), int(cg::grid_fit(512, r0)));
}

static void device_int() {
  cg::DeviceInt d;
  int q = 0;
  auto cus = [&](int dev) { return d.get(dev, [&] { ++q; return dev == 0 ? 256 : dev == 1 ? 128 : -1; }); };
  const int a = cus(0) + cus(0) + cus(0), b = cus(1) + cus(1), c = cus(2) + cus(2);
  printf("device_int %d %d %d %d\n", a, b, c, q);
}

int main() {
  once();
  threads();
  counts();
  device_int();
  return 0;
}
"""


@pytest.fixture(scope="module")
def out(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("g++ not available")
    d = tmp_path_factory.mktemp("launch")
    src = d / "launch.cpp"
    src.write_text(SRC)
    exe = str(d / "launch")
    subprocess.run([gxx, "-O1", "-std=c++17", "-I", HDR, str(src), "-o", exe, "-pthread"],
                   check=True, capture_output=True, timeout=120)
    text = subprocess.run([exe], check=True, capture_output=True, text=True, timeout=30).stdout
    return {l.split()[0]: [int(x) for x in l.split()[1:]] for l in text.splitlines()}


def test_opt_in_once_per_device_and_kernel(out):
    total, one, dev1, kern2, f0, f1, f2, failed_calls, other_dev, far_calls = out["once"]
    assert total == 0  # every call returned the setter's success
    assert one == 1  # 1000 calls, one kernel, one device
    assert dev1 == 1  # the same kernel on a second device
    assert kern2 == 1  # a second kernel
    assert (f0, f1, f2) == (719, 719, 719) and failed_calls == 1
    assert other_dev == 0
    assert far_calls == 2


def test_opt_in_eight_threads_one_key(out):
    set_calls, early, wrong = out["threads"]
    assert set_calls == 1
    assert early == 0  # no thread returned before the setter had
    assert wrong == 0  # every thread saw its status


def test_resident_count_one_query_per_key(out):
    r0, q_one, r1, r2, r3, r4, q_keys, unknown, q_fail = out["counts"]
    assert r0 == 2 * 256 and q_one == 1
    assert r1 == 2 * 128 and r2 == r0 and r3 == r0 and r4 == 4 * 256
    assert q_keys == 5  # (device, kernel, threads, LDS): each its own query
    assert unknown == -1 and q_fail == 1


def test_callers_policies_on_unknown_count(out):
    gemm_unknown, gemm_known, xb_unknown, xb_known, fit_unknown, fit_large, fit_ok = out["policy"]
    assert gemm_unknown == 1024  # the row GEMM keeps its cap
    assert gemm_known == 512
    assert xb_unknown == 256  # k_xbasis: one workgroup per CU on 256 CUs
    assert xb_known == 512
    assert fit_unknown == 2  # kGridUnknown: the residency check refuses
    assert fit_large == 1 and fit_ok == 0


def test_device_int_cached_per_device(out):
    a, b, c, q = out["device_int"]
    assert a == 3 * 256 and b == 2 * 128
    assert c == -2  # a failed query reads -1; the caller keeps its fallback
    assert q == 3  # one query per device, the failed one included
