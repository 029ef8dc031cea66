// optim.hip -- AdamW over flat parameter arenas with global-norm clipping, all scalars on device
// (graph-replay safe): torch.optim.AdamW semantics (train_cape_episodic.py:527-538) after
// torch.nn.utils.clip_grad_norm_(max_norm) (engine_cape.py:240-246).  Pure HBM streaming:
// 4 reads + 3 writes of 4 bytes per parameter.
#include "common.h"

namespace {

// Sum of squares as per-block PARTIAL sums: exactly SUMSQ_PARTS blocks of 16 waves, block b writes out[b] (blocks beyond the data
// write 0).  No float atomics: a reduction whose order depends on block arrival gave two data-parallel replicas -- same all-reduced
// gradient -- clip coefficients one ulp apart, and their parameters drifted from each other step by step (tools/ddp_rehearsal.py).
// The consumer (adamw_kernel) adds the partials in a fixed order.
constexpr int SUMSQ_PARTS = CAPE_SUMSQ_PARTS;
__global__ void __launch_bounds__(1024) sumsq_kernel(const float* g, long long n, float* out) {
  __shared__ float sh[16];
  float s = 0.f;
  const long long n4 = n >> 2;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
    const float4 v = reinterpret_cast<const float4*>(g)[i];
    s += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) { const float v = g[(n4 << 2) + threadIdx.x]; s += v * v; }
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    float a = 0.f;
#pragma unroll
    for (int k = 0; k < 16; ++k) a += sh[k];
    out[blockIdx.x] = a;
  }
}

// GUARDED: the step is applied only while the device flag `bad` (cape_step_guard) is clear -- every block returns before it
// touches p, m, v otherwise.  The flag is uniform over the grid, so the early return precedes the barrier below in all threads.
template <bool GUARDED>
__global__ void __launch_bounds__(256) adamw_kernel(float* p, const float* g, float* m, float* v, long long n, float lr,
                                                     float b1, float b2, float eps, float wd, float max_norm,
                                                     const float* sumsq, int n_parts, const int64_t* step_count, const float* lr_dev,
                                                     const int* bad) {
  if (GUARDED && bad[0] != 0) return;
  if (lr_dev) lr = lr_dev[0];                                // the schedule's value of this step, kept on the device (replayed graphs)
  float coef = 1.f;
  if (max_norm > 0.f) {
    // global gradient norm from the partial sums, the same fixed order in every block (and on every rank)
    __shared__ float tot;
    if (threadIdx.x < 64) {
      float a = 0.f;
      for (int k = threadIdx.x; k < n_parts; k += 64) a += sumsq[k];
      a = wave_sum(a);
      if (threadIdx.x == 0) tot = a;
    }
    __syncthreads();
    coef = fminf(1.f, max_norm / (sqrtf(tot) + 1e-6f));
  }
  const float t = (float)step_count[0];
  const float bc1 = 1.f - powf(b1, t);
  const float bc2s = sqrtf(1.f - powf(b2, t));
  const float step_size = lr / bc1;
  const float decay = 1.f - lr * wd;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const float gi = g[i] * coef;
    float pi = p[i] * decay;
    const float mi = m[i] + (gi - m[i]) * (1.f - b1);     // lerp
    const float vi = v[i] * b2 + gi * gi * (1.f - b2);
    m[i] = mi;
    v[i] = vi;
    pi -= step_size * mi / (sqrtf(vi) / bc2s + eps);
    p[i] = pi;
  }
}

__global__ void step_inc_kernel(int64_t* s) { s[0] += 1; }

__device__ __forceinline__ bool non_finite(float x) { return (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u; }

// One wave.  Books one training iteration on the device (a captured step cannot ask the host): copies the criterion's scalars
// into row (serial % ring_len) of the ring, works out the global gradient norm from the partial sums in adamw_kernel's order
// (lane k adds parts k, k+64, ...; then the wave sum), raises the sticky flag `bad` on a non-finite total or norm and counts
// the optimizer step only while the flag is clear.  Row layout: cape_hip.h.  Plain vector stores, no atomics.
__global__ void __launch_bounds__(64) step_guard_kernel(const float* total, const float* losses, int n_losses, const float* sumsq,
                                                        int n_parts, float max_norm, const float* lr_dev, int64_t* step_count,
                                                        int* serial, int* bad, float* ring, int ring_len, int row_stride) {
  const bool is_step = sumsq != nullptr;
  float norm = CAPE_GUARD_NO_STEP, coef = 1.f;
  if (is_step) {
    float a = 0.f;
    for (int k = threadIdx.x; k < n_parts; k += 64) a += sumsq[k];
    norm = sqrtf(wave_sum(a));
    if (max_norm > 0.f) coef = fminf(1.f, max_norm / (norm + 1e-6f));
  }
  const float tot = total ? total[0] : 0.f;
  const int now_bad = (bad[0] != 0 || non_finite(tot) || (is_step && non_finite(norm))) ? 1 : 0;
  const int ser = serial[0];
  float* row = ring ? ring + (long long)(ser % ring_len) * row_stride : nullptr;
  if (row)
    for (int k = threadIdx.x; k < n_losses; k += 64) row[CAPE_GUARD_ROW_LOSSES + k] = losses[k];
  if (threadIdx.x == 0) {
    if (row) {
      row[CAPE_GUARD_ROW_SERIAL] = __int_as_float(ser);
      row[CAPE_GUARD_ROW_OK] = __int_as_float(now_bad ? 0 : 1);
      row[CAPE_GUARD_ROW_TOTAL] = tot;
      row[CAPE_GUARD_ROW_NORM] = norm;
      row[CAPE_GUARD_ROW_COEF] = coef;
      row[CAPE_GUARD_ROW_LR] = lr_dev[0];
      serial[0] = ser + 1;
    }
    bad[0] = now_bad;
    if (is_step && !now_bad) step_count[0] += 1;
  }
}

}  // namespace

extern "C" int cape_sumsq(const float* g, long long n, float* out, cape_stream_t stream) {
  CAPE_REQUIRE(g && out && n >= 0, "cape_sumsq: bad arguments");
  if (n == 0) return 0;
  CAPE_REQUIRE((reinterpret_cast<uintptr_t>(g) & 15) == 0, "cape_sumsq: g must be 16-byte aligned");
  hipLaunchKernelGGL(sumsq_kernel, dim3(SUMSQ_PARTS), dim3(1024), 0, as_stream(stream), g, n, out);
  CAPE_LAUNCH_CHECK("cape_sumsq");
  return 0;
}

extern "C" int cape_adamw_step(float* p, const float* g, float* m, float* v, long long n, float lr, float beta1, float beta2,
                               float eps, float weight_decay, float max_norm, const float* sumsq, int n_parts,
                               const int64_t* step_count, const float* lr_dev, cape_stream_t stream) {
  CAPE_REQUIRE(p && g && m && v && step_count && n >= 0, "cape_adamw_step: bad arguments");
  CAPE_REQUIRE(max_norm <= 0.f || (sumsq && n_parts >= 1), "cape_adamw_step: clipping needs the partial sums of cape_sumsq");
  if (n == 0) return 0;
  long long b = (n + 255) / 256;
  if (b > 4096) b = 4096;
  hipLaunchKernelGGL(adamw_kernel<false>, dim3((unsigned)b), dim3(256), 0, as_stream(stream), p, g, m, v, n, lr, beta1, beta2, eps,
                     weight_decay, max_norm, sumsq, n_parts, step_count, lr_dev, (const int*)nullptr);
  CAPE_LAUNCH_CHECK("cape_adamw_step");
  return 0;
}

extern "C" int cape_adamw_step_guarded(float* p, const float* g, float* m, float* v, long long n, float lr, float beta1, float beta2,
                                       float eps, float weight_decay, float max_norm, const float* sumsq, int n_parts,
                                       const int64_t* step_count, const float* lr_dev, const int* bad, cape_stream_t stream) {
  CAPE_REQUIRE(p && g && m && v && step_count && bad && n >= 0, "cape_adamw_step_guarded: bad arguments");
  CAPE_REQUIRE(max_norm <= 0.f || (sumsq && n_parts >= 1), "cape_adamw_step_guarded: clipping needs the partial sums of cape_sumsq");
  if (n == 0) return 0;
  long long b = (n + 255) / 256;
  if (b > 4096) b = 4096;
  hipLaunchKernelGGL(adamw_kernel<true>, dim3((unsigned)b), dim3(256), 0, as_stream(stream), p, g, m, v, n, lr, beta1, beta2, eps,
                     weight_decay, max_norm, sumsq, n_parts, step_count, lr_dev, bad);
  CAPE_LAUNCH_CHECK("cape_adamw_step_guarded");
  return 0;
}

extern "C" int cape_step_guard(const float* total, const float* losses, int n_losses, const float* sumsq, int n_parts,
                               float max_norm, const float* lr_dev, int64_t* step_count, int* serial, int* bad, float* ring,
                               int ring_len, int row_stride, cape_stream_t stream) {
  CAPE_REQUIRE(step_count && serial && bad, "cape_step_guard: null pointer");
  CAPE_REQUIRE(!sumsq || n_parts >= 1, "cape_step_guard: an optimizer step needs the partial sums of cape_sumsq");
  if (ring) {
    CAPE_REQUIRE(total && lr_dev && n_losses >= 0 && (losses || n_losses == 0), "cape_step_guard: a row needs total, losses and lr");
    CAPE_REQUIRE(ring_len >= 1 && row_stride >= CAPE_GUARD_ROW_LOSSES + n_losses, "cape_step_guard: row too short for the losses");
  }
  hipLaunchKernelGGL(step_guard_kernel, dim3(1), dim3(64), 0, as_stream(stream), total, losses, n_losses, sumsq, n_parts, max_norm,
                     lr_dev, step_count, serial, bad, ring, ring_len, row_stride);
  CAPE_LAUNCH_CHECK("cape_step_guard");
  return 0;
}

extern "C" int cape_step_increment(int64_t* step_count, cape_stream_t stream) {
  CAPE_REQUIRE(step_count, "cape_step_increment: null pointer");
  hipLaunchKernelGGL(step_inc_kernel, dim3(1), dim3(1), 0, as_stream(stream), step_count);
  CAPE_LAUNCH_CHECK("cape_step_increment");
  return 0;
}
