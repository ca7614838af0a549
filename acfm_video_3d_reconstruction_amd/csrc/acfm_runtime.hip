// What every unit of the library reaches through acfm_common.h: the stream-ordered zero fill (in place of
// hipMemsetAsync) and the profiling ring (prof_begin / prof_end), with the entry points that have no kernel of
// their own -- version, architecture, stream-capture query, acfm_prof_*.
#include "acfm_common.h"

#include <atomic>
#include <mutex>

namespace acfm {

// Zero-fill by a kernel instead of hipMemsetAsync: a memset node in front of k_setup came out
// wrong when the call was captured into a hipGraph and replayed (tests/test_gpu_render.py::
// test_hip_graph_capture_and_replay); kernel nodes replay reliably, so the library uses no memsets.
__global__ void k_zero_bytes(unsigned char* __restrict__ p, size_t nbytes) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t nw = nbytes >> 2;
  if (i < nw) reinterpret_cast<unsigned*>(p)[i] = 0u;
  if (i < (nbytes & 3)) p[(nw << 2) + i] = 0;
}
// large 16-byte-aligned buffers (atlas gradients, the solver's identity rows): 16-byte stores, 4 per thread
__global__ __launch_bounds__(256) void k_zero_vec(uint4* __restrict__ p, size_t n16) {
  const size_t base = (size_t)blockIdx.x * 1024 + threadIdx.x;
  const uint4 z = make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const size_t i = base + 256 * (size_t)k;
    if (i < n16) p[i] = z;
  }
}
int zero_async(void* p, size_t nbytes, hipStream_t st) {
  if (nbytes == 0) return ACFM_OK;
  if (((uintptr_t)p & 3) != 0) return ACFM_E_BADARG;
  if (nbytes >= (1u << 16) && ((uintptr_t)p & 15) == 0) {
    const size_t n16 = nbytes >> 4;
    hipLaunchKernelGGL(k_zero_vec, dim3((unsigned)((n16 + 1023) / 1024)), dim3(256), 0, st, (uint4*)p, n16);
    p = (unsigned char*)p + (n16 << 4);
    nbytes &= 15;
    if (nbytes == 0) return hipGetLastError() == hipSuccess ? ACFM_OK : ACFM_E_LAUNCH;
  }
  const size_t n = (nbytes >> 2) > 4 ? (nbytes >> 2) : 4;
  hipLaunchKernelGGL(k_zero_bytes, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (unsigned char*)p, nbytes);
  return hipGetLastError() == hipSuccess ? ACFM_OK : ACFM_E_LAUNCH;
}

// ------------------------------------------------------------------------------- profiling
// One ring per process, shared by all devices and threads (a measurement aid, off by default): the
// flag is atomic, the ring is guarded by a mutex held from prof_begin to prof_end of a launch.
static std::atomic<bool> g_prof_on{false};
static std::mutex g_prof_mu;
static hipEvent_t g_ev[ACFM_PROF_RING][2];
static int g_ev_id[ACFM_PROF_RING];
static int g_ev_n = 0;
static bool g_ev_made = false;
static thread_local bool t_prof_open = false;

void prof_begin(int id, hipStream_t st) {
  if (!g_prof_on.load(std::memory_order_relaxed)) return;
  g_prof_mu.lock();
  if (!g_prof_on.load() || g_ev_n >= ACFM_PROF_RING) { g_prof_mu.unlock(); return; }
  t_prof_open = true;
  g_ev_id[g_ev_n] = id;
  (void)hipEventRecord(g_ev[g_ev_n][0], st);
}
void prof_end(hipStream_t st) {
  if (!t_prof_open) return;
  (void)hipEventRecord(g_ev[g_ev_n][1], st);
  g_ev_n++;
  t_prof_open = false;
  g_prof_mu.unlock();
}

}  // namespace acfm

using namespace acfm;

extern "C" {

int acfm_version(void) { return 2000; }
const char* acfm_arch(void) { return "gfx950"; }

int acfm_stream_capture_id(void* stream, unsigned long long* id_host) {
  if (!id_host) return ACFM_E_BADARG;
  hipStreamCaptureStatus status = hipStreamCaptureStatusNone;
  unsigned long long id = 0;
  if (hipStreamGetCaptureInfo((hipStream_t)stream, &status, &id) != hipSuccess) return ACFM_E_LAUNCH;
  *id_host = status == hipStreamCaptureStatusActive ? (id ? id : ~0ull) : 0ull;
  return ACFM_OK;
}

int acfm_prof_enable(int on) {
  std::lock_guard<std::mutex> lk(g_prof_mu);
  if (on && !g_ev_made) {
    for (int i = 0; i < ACFM_PROF_RING; ++i)
      if (hipEventCreate(&g_ev[i][0]) != hipSuccess || hipEventCreate(&g_ev[i][1]) != hipSuccess)
        return ACFM_E_LAUNCH;
    g_ev_made = true;
  }
  g_ev_n = 0;
  g_prof_on = on != 0;
  return ACFM_OK;
}

int acfm_prof_collect(float* ms_host, int* count_host, int n) {
  if (!ms_host || !count_host || n < ACFM_PROF_NKERNELS) return ACFM_E_BADARG;
  std::lock_guard<std::mutex> lk(g_prof_mu);
  for (int i = 0; i < n; ++i) { ms_host[i] = 0.f; count_host[i] = 0; }
  for (int i = 0; i < g_ev_n; ++i) {
    if (hipEventSynchronize(g_ev[i][1]) != hipSuccess) return ACFM_E_LAUNCH;
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, g_ev[i][0], g_ev[i][1]) != hipSuccess) return ACFM_E_LAUNCH;
    ms_host[g_ev_id[i]] += ms;
    count_host[g_ev_id[i]] += 1;
  }
  g_ev_n = 0;
  return ACFM_OK;
}

const char* acfm_prof_name(int id) {
  static const char* names[ACFM_PROF_NKERNELS] = {
      "k_setup", "k_raster_fwd<K,soft>", "k_sil_bwd", "k_project_bwd", "k_raster_fwd<1,tex>",
      "k_raster_fwd<1,hard>", "k_tex_bwd", "k_mask_losses", "k_mask_losses_bwd", "k_visible",
      "k_bds_loss", "k_bds_loss_bwd", "k_project", "k_tex_mse", "k_tex_mse_bwd", "k_deform_apply",
      "k_deform_bwd", "deform_solve", "deform_solve_bwd", "fragments_fwd", "k_frag_bwd", "k_boundary_subset", "k_step_tail", ""};
  return (id >= 0 && id < ACFM_PROF_NKERNELS) ? names[id] : "";
}

}  // extern "C"
