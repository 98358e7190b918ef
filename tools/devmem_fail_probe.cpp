// devmem_fail_probe.cpp -- the failure path of csrc/lt_devmem.h, run where every hipMalloc fails: on a host WITHOUT a GPU
// (hipMalloc returns hipErrorNoDevice and leaves the pointer alone).  Checks what a failed replacement leaves behind: a
// non-LT_OK return, every pointer of the group NULL, the capacity 0, lt_last_error() naming the caller.  With a GPU the
// allocations succeed and the program says so and proves nothing.  Host code under AddressSanitizer + UBSan, stand-alone:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -I include -I lidar_transfer_amd/csrc \
//         -o /tmp/devmem_fail_probe tools/devmem_fail_probe.cpp && /tmp/devmem_fail_probe
#include <stdarg.h>
#include <stdio.h>
#include <string.h>
#include "lt_devmem.h"

static char g_err[512] = "";
void lt_set_error(const char* fmt, ...) {  // (the library's is in lt_api.hip)
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}
extern "C" const char* lt_last_error(void) { return g_err; }

static int g_bad = 0;
#define EXPECT(cond)                                              \
  do {                                                            \
    if (!(cond)) { printf("  FAILED: %s (line %d)\n", #cond, __LINE__); ++g_bad; } \
  } while (0)

static void report(const char* what, int rc) { printf("%s: rc=%d, \"%s\"\n", what, rc, lt_last_error()); }

int main() {
  int n_dev = 0;
  if (hipGetDeviceCount(&n_dev) == hipSuccess && n_dev > 0) {
    printf("a GPU is present: allocations succeed here, nothing to probe\n");
    return 2;
  }
  (void)hipGetLastError();
  {  // a group of three that never existed (an empty group), int capacity
    float* a = nullptr; int* b = nullptr; double* c = nullptr;
    int cap = 0;
    const lt_dev_array g[] = {{(void**)&a, 1000 * sizeof(float)}, {(void**)&b, 1000 * sizeof(int)}, {(void**)&c, 1000 * sizeof(double)}};
    const int rc = lt_dev_replace("probe_group_of_three", lt_wait_device(), &cap, 1000, g);
    report("group of three, empty, device wait", rc);
    EXPECT(rc != LT_OK); EXPECT(!a && !b && !c); EXPECT(cap == 0); EXPECT(strstr(lt_last_error(), "probe_group_of_three"));
    EXPECT(strstr(lt_last_error(), "4000 bytes"));
  }
  {  // the same group behind a stale capacity: a failed replacement must not leave it standing
    float* a = nullptr; int* b = nullptr; double* c = nullptr;
    size_t cap = 777;
    const lt_dev_array g[] = {{(void**)&a, 64}, {(void**)&b, 0}, {(void**)&c, 4096}};  // (0 bytes: dropped, not allocated)
    const int rc = lt_dev_replace("probe_stale_capacity", lt_wait_stream(nullptr), &cap, (size_t)2000, g);
    report("group of three, stale capacity, stream wait", rc);
    EXPECT(rc != LT_OK); EXPECT(!a && !b && !c); EXPECT(cap == 0); EXPECT(strstr(lt_last_error(), "probe_stale_capacity"));
  }
  {  // a group without a capacity of its own
    unsigned* a = nullptr; unsigned* b = nullptr; unsigned* c = nullptr;
    const lt_dev_array g[] = {{(void**)&a, 16}, {(void**)&b, 16}, {(void**)&c, 16}};
    const int rc = lt_dev_replace("probe_no_capacity", lt_wait_none(), g);
    report("group of three, no capacity, no wait", rc);
    EXPECT(rc != LT_OK); EXPECT(!a && !b && !c); EXPECT(strstr(lt_last_error(), "probe_no_capacity"));
  }
  {  // the one-array form, empty, with the headroom rule
    float* p = nullptr;
    size_t cap = 0;
    const int rc = lt_dev_grow("probe_one_array", lt_wait_device(), &p, &cap, 100, lt_headroom(100));
    report("one array, empty", rc);
    EXPECT(rc != LT_OK); EXPECT(!p); EXPECT(cap == 0); EXPECT(strstr(lt_last_error(), "probe_one_array"));
    EXPECT(lt_headroom(100) == 1149);
  }
  {  // the one-array form behind a stale capacity that would hold the demand: no pointer, so it allocates (and fails)
    int* p = nullptr;
    int cap = 5000;
    const int rc = lt_dev_grow("probe_one_array_stale", lt_wait_none(), &p, &cap, 100, 100);
    report("one array, stale capacity", rc);
    EXPECT(rc != LT_OK); EXPECT(!p); EXPECT(cap == 0); EXPECT(strstr(lt_last_error(), "probe_one_array_stale"));
  }
  printf(g_bad ? "%d checks FAILED\n" : "all checks passed\n", g_bad);
  return g_bad ? 1 : 0;
}
