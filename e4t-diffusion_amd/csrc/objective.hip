// The training objective on fp32 latents: e4t_diffuse forms the noisy input, the target and the per-image loss weight in one pass, and the
// masked, weighted (min-SNR) and robust (pseudo-Huber / smooth-L1) losses reduce in two deterministic stages and share one backward.
// Compiled with the library's common flags only: diffuse_kernel's comment relies on -ffp-contract=fast being a property of this file.
#include "common.h"
#include "../../include/e4t_hip.h"

// ---- masked diffusion loss (the reference's README.md:112-115 TODO on the loss of pretrain_e4t.py:645-647) ----
// loss = sum_{b,c,p} w[b][p] * d^2 / den,  d = pred - target,  den = C * max(sum(w), 1);  dpred = g * 2 * w * d / den.
// Two-stage reductions in a fixed order (per-thread pixel stride, block_sum, then one block over the partials): no atomics, so a
// result is bitwise the same from run to run.  Forward = partial + final, backward = one streaming pass over the saved w * d.
namespace {
constexpr int MMSE_MAX_BLOCKS = 1024;

// one thread per pixel (b, p), all C channels: w is read once, sum(w) falls out of the same pass.  wd (pred's layout, may be null) = w * d.
// WEIGHTED (e4t_weighted_mse_fwd): w may be null (all ones) and the pixel's weight on d is lam[b] * w (lam may be null: all ones), while
// sum(w) — the normaliser — stays the mask's alone; wd = lam * w * d.  WEIGHTED = false is the masked loss, operation for operation.
template <bool WEIGHTED>
__global__ __launch_bounds__(256) void masked_mse_partial_kernel(const float* __restrict__ pred, const float* __restrict__ target, const float* __restrict__ w,
                                                                 const float* __restrict__ lam, float* __restrict__ wd, float* __restrict__ partial,
                                                                 int B, int C, int HW, int nhwc) {
  __shared__ float red[32];
  const long long npix = (long long)B * HW;
  float se = 0.f, sw = 0.f;
  for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < npix; q += (long long)gridDim.x * 256) {
    const long long b = q / HW;
    const int p = (int)(q - b * HW);
    float wq = (WEIGHTED && !w) ? 1.f : w[q];
    sw += wq;
    if (WEIGHTED && lam) wq = lam[b] * wq;
    for (int c = 0; c < C; ++c) {
      const long long it = (b * C + c) * HW + p;
      const long long ip = nhwc ? q * C + c : it;
      const float d = pred[ip] - target[it];
      const float v = wq * d;
      if (wd) wd[ip] = v;
      se = fmaf(v, d, se);
    }
  }
  se = block_sum(se, red);
  sw = block_sum(sw, red + 16);
  if (threadIdx.x == 0) { partial[blockIdx.x] = se; partial[gridDim.x + blockIdx.x] = sw; }
}
// out[0] = loss, out[1] = den
__global__ __launch_bounds__(256) void masked_mse_final_kernel(const float* __restrict__ partial, int nb, int C, float* __restrict__ out) {
  __shared__ float red[32];
  float se = 0.f, sw = 0.f;
  for (int i = threadIdx.x; i < nb; i += 256) { se += partial[i]; sw += partial[nb + i]; }
  se = block_sum(se, red);
  sw = block_sum(sw, red + 16);
  if (threadIdx.x == 0) {
    const float den = (float)C * fmaxf(sw, 1.f);
    out[0] = se / den;
    out[1] = den;
  }
}
__global__ __launch_bounds__(256) void masked_mse_bwd_kernel(const float* __restrict__ wd, const float* __restrict__ stats, const float* __restrict__ g,
                                                             float* __restrict__ dpred, long long n) {
  const float k = g[0] * 2.f / stats[1];
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) dpred[i] = k * wd[i];
}

// The scheduled pseudo-Huber / smooth-L1 loss (e4t_robust_loss_fwd): masked_mse_partial_kernel<true>'s sibling, the same
// pixel walk and the same two partial rows, so masked_mse_final_kernel finishes it.  Per image c = ctab[t] (t = timesteps[b] clamped into
// the table as diffuse_kernel clamps it; timesteps null = ctab[0]) and, with r = sqrt(d^2 + c^2), h = d^2 / (r + c) — which is r - c
// without the cancellation that costs the textbook form up to 2e-2 at c = 1e3 —
//   huber (kind 1): l = 2 c h, dl/dd = 2 c d / r;   smooth_l1 (kind 2): l = 2 h, dl/dd = 2 d / r.
// With kh = k / 2 = c | 1 the row sums 2 * lam * w * kh * h and wd = lam * w * kh * d / r, half the gradient's numerator, which is what
// masked_mse_bwd_kernel (g * 2 / den * wd) expects.  sqrtf and `/` are the IEEE ones; d == 0 gives h = 0 and wd = 0 as c > 0.
__global__ __launch_bounds__(256) void robust_loss_partial_kernel(const float* __restrict__ pred, const float* __restrict__ target, const float* __restrict__ w,
                                                                  const float* __restrict__ lam, const float* __restrict__ ctab,
                                                                  const long long* __restrict__ timesteps, float* __restrict__ wd,
                                                                  float* __restrict__ partial, int B, int C, int HW, int T, int kind, int nhwc) {
  __shared__ float red[32];
  const long long npix = (long long)B * HW;
  float se = 0.f, sw = 0.f;
  for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < npix; q += (long long)gridDim.x * 256) {
    const long long b = q / HW;
    const int p = (int)(q - b * HW);
    long long t = timesteps ? timesteps[b] : 0;
    t = t < 0 ? 0 : (t > T - 1 ? T - 1 : t);
    const float cb = ctab[t], c2 = cb * cb;
    float wq = w ? w[q] : 1.f;
    sw += wq;
    if (lam) wq = lam[b] * wq;
    if (kind == 1) wq = wq * cb;                              // lam * w * k / 2
    const float wq2 = 2.f * wq;
    for (int c = 0; c < C; ++c) {
      const long long it = (b * C + c) * HW + p;
      const long long ip = nhwc ? q * C + c : it;
      const float d = pred[ip] - target[it];
      const float d2 = d * d;
      const float r = sqrtf(d2 + c2);
      if (wd) wd[ip] = wq * d / r;
      se = fmaf(wq2, d2 / (r + cb), se);
    }
  }
  se = block_sum(se, red);
  sw = block_sum(sw, red + 16);
  if (threadIdx.x == 0) { partial[blockIdx.x] = se; partial[gridDim.x + blockIdx.x] = sw; }
}

// ---- host side of the three forward entries: stats = {loss, den} + the two partial rows of nb blocks each ----
static_assert(E4T_MASKED_MSE_STATS == 2 + 2 * MMSE_MAX_BLOCKS, "stats = {loss, den} + the two partial rows");
int loss_blocks(int B, int HW) { return (int)min(cdivl((long long)B * HW, 256), (long long)MMSE_MAX_BLOCKS); }
int finish_loss(float* stats, int nb, int C, hipStream_t s) {
  hipLaunchKernelGGL(masked_mse_final_kernel, dim3(1), dim3(256), 0, s, (const float*)(stats + 2), nb, C, stats);
  E4T_CHECK_LAUNCH("masked_mse_final_kernel");
  return 0;
}
}  // namespace

extern "C" int e4t_masked_mse_fwd(const float* pred, const float* target, const float* w, float* wd, float* stats, int B, int C, int HW, int pred_nhwc, e4t_stream s) {
  E4T_REQUIRE(pred && target && w && stats && B > 0 && C > 0 && HW > 0, "masked_mse_fwd: bad arguments");
  const int nb = loss_blocks(B, HW);
  hipLaunchKernelGGL(masked_mse_partial_kernel<false>, dim3(nb), dim3(256), 0, (hipStream_t)s, pred, target, w, (const float*)nullptr, wd, stats + 2, B, C, HW, pred_nhwc);
  E4T_CHECK_LAUNCH("masked_mse_partial_kernel");
  return finish_loss(stats, nb, C, (hipStream_t)s);
}
// the same two launches with a per-image weight lam[B] and an optional mask (min-SNR weighting); the backward is
// e4t_masked_mse_bwd on the saved lam * w * d, whose arithmetic (g * 2 / den * wd) is already the weighted gradient's
extern "C" int e4t_weighted_mse_fwd(const float* pred, const float* target, const float* w, const float* lam, float* wd, float* stats, int B, int C, int HW, int pred_nhwc,
                                    e4t_stream s) {
  E4T_REQUIRE(pred && target && stats && B > 0 && C > 0 && HW > 0, "weighted_mse_fwd: bad arguments (pred, target, stats non-null; B, C, HW > 0)");
  const int nb = loss_blocks(B, HW);
  hipLaunchKernelGGL(masked_mse_partial_kernel<true>, dim3(nb), dim3(256), 0, (hipStream_t)s, pred, target, w, lam, wd, stats + 2, B, C, HW, pred_nhwc);
  E4T_CHECK_LAUNCH("weighted_mse_partial_kernel");
  return finish_loss(stats, nb, C, (hipStream_t)s);
}
// the scheduled pseudo-Huber / smooth-L1 loss in the same two launches; the backward is e4t_masked_mse_bwd on the saved
// lam * w * (k / 2) * d / r, as for the weighted loss
extern "C" int e4t_robust_loss_fwd(const float* pred, const float* target, const float* w, const float* lam, const float* ctab, const long long* timesteps, float* wd,
                                   float* stats, int B, int C, int HW, int T, int kind, int pred_nhwc, e4t_stream s) {
  E4T_REQUIRE(pred && target && ctab && stats && B > 0 && C > 0 && HW > 0, "robust_loss_fwd: bad arguments (pred, target, ctab, stats non-null; B, C, HW > 0)");
  E4T_REQUIRE(T >= 1, "robust_loss_fwd: T = %d, the table needs at least one entry", T);
  E4T_REQUIRE(kind == E4T_LOSS_HUBER || kind == E4T_LOSS_SMOOTH_L1, "robust_loss_fwd: kind = %d must be 1 (huber) or 2 (smooth_l1)", kind);
  const int nb = loss_blocks(B, HW);
  hipLaunchKernelGGL(robust_loss_partial_kernel, dim3(nb), dim3(256), 0, (hipStream_t)s, pred, target, w, lam, ctab, timesteps, wd, stats + 2, B, C, HW, T, kind, pred_nhwc);
  E4T_CHECK_LAUNCH("robust_loss_partial_kernel");
  return finish_loss(stats, nb, C, (hipStream_t)s);
}
extern "C" int e4t_masked_mse_bwd(const float* wd, const float* stats, const float* g, float* dpred, long long n, e4t_stream s) {
  E4T_REQUIRE(wd && stats && g && dpred && n > 0, "masked_mse_bwd: bad arguments");
  hipLaunchKernelGGL(masked_mse_bwd_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)s, wd, stats, g, dpred, n);
  E4T_CHECK_LAUNCH("masked_mse_bwd_kernel");
  return 0;
}

// ---- the diffusion objective's inputs in one pass (trainer.py add_noise + the target lines) ----
//   n' = noise + s * z[b][c]  (only with an offset: z null = n' is noise itself),  noisy = a*x0 + sg*n',
//   target = n' (epsilon) | a*n' - sg*x0 (v-prediction),  lam[b] = coef[t][2],  {a, sg} = coef[t][0..1],  t = timesteps[b] clamped to the table.
// Every product, sum and difference is rounded on its own, in the order of the torch expressions, so the outputs are those of the stock
// elementwise ops bit for bit.  hipcc's __fmul_rn / __fadd_rn / __fsub_rn are plain `*`, `+`, `-`, which this file's -ffp-contract=fast
// contracts into an FMA like any other (the float4 kernel came out as v_pk_fma_f32: up to 120 ulp from torch where the two products
// cancel), and under that flag `#pragma clang fp contract(off)` is ignored.  So every product goes through mul_rn: the canonicalize
// behind the multiply is dropped at instruction selection (a product is canonical already, it costs no instruction) but leaves the
// combiner no multiply next to the sum or difference to fuse with.  Every sum / difference here has such products as its operands.
// V = 4: HW % 4 == 0 and 16-byte aligned tensors, a float4 never crosses a (b, c) row; V = 1 otherwise.
namespace {
__device__ __forceinline__ float mul_rn(float a, float b) { return __builtin_canonicalizef(a * b); }
__device__ __forceinline__ void diffuse_f(float x, float nz, bool offs, float off, float a, float sg, int vpred, float& ny, float& tg) {
  const float n1 = offs ? nz + off : nz;                     // off = mul_rn(s, z)
  ny = mul_rn(a, x) + mul_rn(sg, n1);
  tg = vpred ? mul_rn(a, n1) - mul_rn(sg, x) : n1;
}
template <int V>
__global__ __launch_bounds__(256) void diffuse_kernel(const float* __restrict__ x0, const float* __restrict__ noise, const float* __restrict__ z,
                                                      const long long* __restrict__ timesteps, const float* __restrict__ coef, float* __restrict__ noisy,
                                                      float* __restrict__ target, float* __restrict__ lam, int B, int C, int HW, int T, float s, int vpred) {
  const int rowg = HW / V;                                   // groups of V elements per (b, c) row
  const long long ng = (long long)B * C * rowg;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < ng; i += (long long)gridDim.x * 256) {
    const long long r = i / rowg;                            // row b * C + c
    const int b = (int)(r / C);
    long long t = timesteps[b];
    t = t < 0 ? 0 : (t > T - 1 ? T - 1 : t);
    const float a = coef[3 * t], sg = coef[3 * t + 1];
    if (i == (long long)b * C * rowg) lam[b] = coef[3 * t + 2];
    const bool offs = z != nullptr;
    const float off = offs ? mul_rn(s, z[r]) : 0.f;
    if (V == 4) {
      const float4 X = *(const float4*)(x0 + i * 4), N = *(const float4*)(noise + i * 4);
      float4 Y, G;
      diffuse_f(X.x, N.x, offs, off, a, sg, vpred, Y.x, G.x);
      diffuse_f(X.y, N.y, offs, off, a, sg, vpred, Y.y, G.y);
      diffuse_f(X.z, N.z, offs, off, a, sg, vpred, Y.z, G.z);
      diffuse_f(X.w, N.w, offs, off, a, sg, vpred, Y.w, G.w);
      *(float4*)(noisy + i * 4) = Y;
      *(float4*)(target + i * 4) = G;
    } else {
      float y, g;
      diffuse_f(x0[i], noise[i], offs, off, a, sg, vpred, y, g);
      noisy[i] = y;
      target[i] = g;
    }
  }
}
}  // namespace

extern "C" int e4t_diffuse(const float* x0, const float* noise, const float* z, const long long* timesteps, const float* coef, float* noisy, float* target, float* lam, int B,
                           int C, int HW, int T, float s, int v_prediction, e4t_stream st) {
  E4T_REQUIRE(x0 && noise && timesteps && coef && noisy && target && lam, "diffuse: null pointer (only z may be null)");
  E4T_REQUIRE(B > 0 && C > 0 && HW > 0 && T > 0, "diffuse: B = %d, C = %d, HW = %d, T = %d must be positive", B, C, HW, T);
  E4T_REQUIRE(z || s == 0.f, "diffuse: a noise offset s = %g needs z", (double)s);
  E4T_REQUIRE(s >= 0.f, "diffuse: the noise offset s = %g must be >= 0", (double)s);
  if (s == 0.f) z = nullptr;                                 // no offset term at all: n' is noise itself, not noise + 0 * z
  const long long n = (long long)B * C * HW;
  const bool vec = HW % 4 == 0 && (((uintptr_t)x0 | (uintptr_t)noise | (uintptr_t)noisy | (uintptr_t)target) & 15) == 0;
  hipLaunchKernelGGL(vec ? diffuse_kernel<4> : diffuse_kernel<1>, dim3(grid_for(vec ? n / 4 : n)), dim3(256), 0, (hipStream_t)st, x0, noise, z, timesteps, coef, noisy, target,
                     lam, B, C, HW, T, s, v_prediction);
  E4T_CHECK_LAUNCH("diffuse_kernel");
  return 0;
}
