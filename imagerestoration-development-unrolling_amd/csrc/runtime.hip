// Host runtime shared by every translation unit of libgrr.so: the thread-local error state and launch
// status (grr_last_error), the device queries and size helpers of the launchers, and the scratch leases
// behind the fixed-order reductions (RedScratch, grr_common.h) with the kernel that finishes them.
#include <algorithm>
#include <cstdarg>
#include <mutex>
#include <string>
#include <vector>

#include "grr_device.h"

namespace grr {

static thread_local std::string g_err;

void set_error(const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_err = buf;
}

void clear_error() { g_err.clear(); }

grr_status launch_status(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error("%s: %s", what, hipGetErrorString(e));
    return GRR_ERR_HIP;
  }
  return GRR_OK;
}

// compute units of the current device (cached per device)
int num_cus() {
  static int cache[64] = {};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
  if (!cache[dev]) {
    int n = 0;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
    cache[dev] = n;
  }
  return cache[dev];
}

// workspace regions start on 256-byte boundaries (n floats -> a multiple of 64)
int64_t align64(int64_t n) { return (n + 63) / 64 * 64; }

namespace {

// dst[i] += sum_s part[i][s] for every planned reduction of a launch, slots in order: lane l adds
// slots l, l + 64, ... in order, then the fixed shuffle tree.   grid (sum of n), one wave per value
struct RedFinishArgs {
  const float* part[RedScratch::kMax];
  float* dst[RedScratch::kMax];
  uint32_t nslot[RedScratch::kMax];
  int first[RedScratch::kMax + 1];   // value ranges of the reductions in the grid
  int k;
};
__global__ __launch_bounds__(64) void red_finish_kernel(RedFinishArgs a) {
  int i = 0;
  while (i + 1 < a.k && (int)blockIdx.x >= a.first[i + 1]) ++i;
  const int idx = blockIdx.x - a.first[i];
  const uint32_t nslot = a.nslot[i];
  const float* row = a.part[i] + (size_t)idx * nslot;
  float v = 0.f;
  for (uint32_t s = threadIdx.x; s < nslot; s += 64) v += row[s];
  v = wave_sum(v);
  if (threadIdx.x == 0) a.dst[i][idx] += v;
}

// ---- RedScratch (grr_common.h) ---------------------------------------------
// Scratch leases.  Each (device, stream) owns grow-only buffers, each leased by one RedScratch at a time
// (alloc() to finish()); normally one per stream, a second one only while a lease is nested inside
// another on the same stream.  Later calls on the same stream reuse a buffer: their kernels run after
// the earlier finish kernel in stream order.  Memory comes from the allocator registered by
// grr_set_scratch_allocator (the Python package registers PyTorch's caching allocator, so the scratch
// is visible to and reclaimable through torch), else from hipMalloc / hipFree.  An outgrown buffer is
// retired, not freed (a queued kernel may still read it), until grr_release_scratch.
// A lease taken while its stream is being captured into a HIP graph is the graph's own: a
// hipMallocAsync / hipFreeAsync pair on the capturing stream (memory nodes of the graph), never one of
// the stream's buffers, so replays do not share memory with eager calls on that stream or with another
// graph, and grr_release_scratch cannot free memory a graph still points at.
struct ScratchBuf {
  int dev;
  hipStream_t s;
  void* p;
  size_t bytes;
  bool cb;        // from the registered allocator
  bool leased;
};
struct ScratchState {
  grr_scratch_alloc_fn alloc = nullptr;
  grr_scratch_free_fn free = nullptr;
  void* ctx = nullptr;
  std::vector<ScratchBuf> bufs;      // live buffers, by (device, stream)
  std::vector<ScratchBuf> retired;   // outgrown, freed by grr_release_scratch
  size_t total = 0;
};
ScratchState g_scratch;
std::mutex g_scratch_mu;
struct CaptureLease {
  void* p;
  hipStream_t s;
};
std::vector<CaptureLease> g_capture_leases;   // leased inside a stream capture, freed by scratch_return

grr_status scratch_raw_alloc(int dev, hipStream_t s, size_t bytes, ScratchBuf* out, const char* what) {
  void* p = nullptr;
  bool cb = false;
  if (g_scratch.alloc) {
    p = g_scratch.alloc((uint64_t)bytes, dev, (void*)s, g_scratch.ctx);
    cb = true;
  } else if (hipMalloc(&p, bytes) != hipSuccess) {
    p = nullptr;
  }
  if (!p) {
    set_error("%s: reduction scratch of %zu bytes: allocation failed", what, bytes);
    return GRR_ERR_HIP;
  }
  *out = ScratchBuf{dev, s, p, bytes, cb, false};
  g_scratch.total += bytes;
  return GRR_OK;
}
void scratch_raw_free(const ScratchBuf& b) {
  if (b.cb) {
    if (g_scratch.free) g_scratch.free(b.p, b.dev, (void*)b.s, g_scratch.ctx);
  } else {
    (void)hipFree(b.p);
  }
  g_scratch.total -= b.bytes;
}

// lease >= bytes for stream s (returned by scratch_return)
grr_status scratch_lease(hipStream_t s, size_t bytes, void** out, const char* what) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) {
    set_error("%s: hipGetDevice failed", what);
    return GRR_ERR_HIP;
  }
  std::lock_guard<std::mutex> lk(g_scratch_mu);
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  GRR_REQUIRE(hipStreamIsCapturing(s, &cap) == hipSuccess && cap != hipStreamCaptureStatusInvalidated,
              GRR_ERR_HIP, "%s: the stream's capture state is invalid", what);
  if (cap == hipStreamCaptureStatusActive) {
    void* p = nullptr;
    if (hipMallocAsync(&p, std::max<size_t>(bytes, 256), s) != hipSuccess || !p) {
      set_error("%s: reduction scratch of %zu bytes inside a stream capture: hipMallocAsync failed", what, bytes);
      return GRR_ERR_HIP;
    }
    g_capture_leases.push_back(CaptureLease{p, s});
    *out = p;
    return GRR_OK;
  }
  ScratchBuf* small = nullptr;
  for (auto& b : g_scratch.bufs) {
    if (b.dev != dev || b.s != s || b.leased) continue;
    if (b.bytes >= bytes) {
      b.leased = true;
      *out = b.p;
      return GRR_OK;
    }
    small = &b;
  }
  size_t want = std::max<size_t>(bytes, (size_t)1 << 20);
  if (small) want = std::max(want, 2 * small->bytes);
  ScratchBuf nb{};
  grr_status st = scratch_raw_alloc(dev, s, want, &nb, what);
  if (st != GRR_OK) return st;
  nb.leased = true;
  if (small) {   // outgrown: retired (queued kernels may still read it), replaced
    g_scratch.retired.push_back(*small);
    *small = nb;
  } else {       // first lease on this stream, or nested inside a live one
    g_scratch.bufs.push_back(nb);
  }
  *out = nb.p;
  return GRR_OK;
}
void scratch_return(void* p) {
  std::lock_guard<std::mutex> lk(g_scratch_mu);
  for (size_t i = 0; i < g_capture_leases.size(); ++i)
    if (g_capture_leases[i].p == p) {   // after the finish kernel on the capturing stream: a free node
      (void)hipFreeAsync(p, g_capture_leases[i].s);
      g_capture_leases.erase(g_capture_leases.begin() + (std::ptrdiff_t)i);
      return;
    }
  for (auto& b : g_scratch.bufs)
    if (b.p == p) b.leased = false;
}
}  // namespace

int RedScratch::plan(float* dst, int n, uint32_t nslot) {
  const int i = k_++;
  dst_[i] = dst;
  n_[i] = n;
  nslot_[i] = nslot < 1 ? 1 : nslot;
  return i;
}

grr_status RedScratch::alloc(const char* what) {
  size_t total = 0;
  for (int i = 0; i < k_; ++i)
    if (dst_[i]) total += (size_t)n_[i] * nslot_[i];
  if (total == 0) return GRR_OK;
  grr_status st = scratch_lease(s_, total * sizeof(float), &base_, what);
  if (st != GRR_OK) {
    base_ = nullptr;
    return st;
  }
  float* p = static_cast<float*>(base_);
  for (int i = 0; i < k_; ++i)
    if (dst_[i]) {
      part_[i] = p;
      p += (size_t)n_[i] * nslot_[i];
    }
  // no fill: every contributor of a launch stores its slot (zero partials included)
  return GRR_OK;
}

grr_status RedScratch::finish(const char* what) {
  RedFinishArgs a{};
  int total = 0;
  for (int i = 0; i < k_; ++i)
    if (dst_[i] && part_[i] && n_[i] > 0) {
      a.part[a.k] = part_[i];
      a.dst[a.k] = dst_[i];
      a.nslot[a.k] = nslot_[i];
      a.first[a.k] = total;
      total += n_[i];
      ++a.k;
    }
  a.first[a.k] = total;
  if (total > 0) hipLaunchKernelGGL(red_finish_kernel, dim3(total), dim3(64), 0, s_, a);
  grr_status st = launch_status(what);
  if (base_) {
    scratch_return(base_);
    base_ = nullptr;
  }
  return st;
}

RedScratch::~RedScratch() {
  if (base_) scratch_return(base_);   // an error path before finish(): nothing was added
}

}  // namespace grr

using namespace grr;

extern "C" {

const char* grr_last_error(void) { return g_err.c_str(); }

grr_status grr_set_scratch_allocator(grr_scratch_alloc_fn alloc, grr_scratch_free_fn free_fn, void* ctx) {
  clear_error();
  GRR_REQUIRE((alloc == nullptr) == (free_fn == nullptr), GRR_ERR_INVALID_ARG,
              "grr_set_scratch_allocator: give both functions or neither");
  std::lock_guard<std::mutex> lk(g_scratch_mu);
  // buffers already handed out stay with the allocator that made them (ScratchBuf::cb); a buffer made
  // by the previous registered allocator is freed through the new one only if that is the same pair
  g_scratch.alloc = alloc;
  g_scratch.free = free_fn;
  g_scratch.ctx = ctx;
  return GRR_OK;
}

grr_status grr_release_scratch(void) {
  clear_error();
  std::lock_guard<std::mutex> lk(g_scratch_mu);
  for (const auto& b : g_scratch.bufs)
    GRR_REQUIRE(!b.leased, GRR_ERR_INVALID_ARG, "grr_release_scratch: a reduction scratch is in use");
  for (const auto& b : g_scratch.bufs) scratch_raw_free(b);
  for (const auto& b : g_scratch.retired) scratch_raw_free(b);
  g_scratch.bufs.clear();
  g_scratch.retired.clear();
  return GRR_OK;
}

int64_t grr_scratch_bytes(void) {
  std::lock_guard<std::mutex> lk(g_scratch_mu);
  return (int64_t)g_scratch.total;
}

}  // extern "C"
