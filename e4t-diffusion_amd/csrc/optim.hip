// The optimiser on flat fp32 buffers: fused AdamW (plain, with the weights' EMA in the same pass, with block-wise 8-bit moments, or with the gradient of the E4T
// head's stacked weights formed in registers from its rank-K factors), the EMA rule alone, and the sum of squares behind the gradient norm.
// Compiled with the library's common flags only: adamw8_kernel's comments rely on -ffp-contract=fast being a property of this file.
#include "common.h"
#include "../../include/e4t_hip.h"

namespace {

// ---- fused AdamW over a flat fp32 buffer (torch.optim.AdamW semantics: decoupled weight decay) ----
// hyper != nullptr: lr, bc1, bc2_sqrt and the gradient scale are read from DEVICE memory ([4] floats) instead of the launch arguments,
// so that a captured (hipGraph) training step replays with the values of ITS step (e4t_adamw_hyper); same arithmetic either way.
// EMA of the weights in the same pass (adamw_ema_kernel): 36 B per parameter instead of 28 + 12 for a pass of its own.  One body, included
// into both kernels (adamw_kernel.inc).
__global__ __launch_bounds__(256) void adamw_kernel(float* p, const float* g, float* m, float* v, long long n, float lr, float b1, float b2,
                                                    float eps, float wd, float bc1, float bc2_sqrt, float gscale, const float* hyper) {
  constexpr bool EMA = false;
  float* const ema = nullptr;
  float ema_w = 0.f;
#include "adamw_kernel.inc"
}
__global__ __launch_bounds__(256) void adamw_ema_kernel(float* p, const float* g, float* m, float* v, float* ema, long long n, float lr, float b1,
                                                        float b2, float eps, float wd, float bc1, float bc2_sqrt, float gscale, float ema_w,
                                                        const float* hyper) {
  constexpr bool EMA = true;
#include "adamw_kernel.inc"
}

// the EMA rule alone, for weights that something else updated (a stock optimiser over the native modules); w_dev != nullptr: w from device memory
__global__ __launch_bounds__(256) void ema_update_kernel(float* ema, const float* p, long long n, float w, const float* w_dev) {
  if (w_dev) w = w_dev[0];
  for (long long i = ((long long)blockIdx.x * 256 + threadIdx.x) * 4; i < n; i += (long long)gridDim.x * 1024) {
    if (i + 4 <= n) {
      const float4 E = *(float4*)(ema + i), P = *(const float4*)(p + i);
      *(float4*)(ema + i) = make_float4(ema_f(E.x, P.x, w), ema_f(E.y, P.y, w), ema_f(E.z, P.z, w), ema_f(E.w, P.w, w));
    } else {
      for (long long j = i; j < n; ++j) ema[j] = ema_f(ema[j], p[j], w);
    }
  }
}

// ---- AdamW with block-wise 8-bit moments (the format is DEFINED by e4t/optimization.py: quantize_blockwise) ----
// m and v live as one byte each (an index into a sorted 256-entry codebook: signed for m, unsigned for v) plus one fp32 scale per 256
// elements: 16.06 B of HBM traffic per parameter instead of 28 (24.06 / 36 with the EMA) -- though as measured the kernel is bound by its per-element
// work (divisions, the two searches), not by HBM, and buys memory rather than time.  One wave64 owns one 256-element block, four
// consecutive elements per lane (a float4 of p and g, one packed word of each code buffer); the block maxima are wave reductions, so
// there is no barrier in the loop.  Per workgroup the two codebooks sit in LDS twice: sorted (dequantisation, the neighbour comparison)
// and as an implicit search tree in breadth-first order (node k's children are 2k and 2k + 1), whose level l occupies 2^l consecutive
// words: the eight reads of a search then fall on distinct banks or on one address, where a binary search over the sorted table would
// read words 128 / 64 / 32 apart (one bank) in its first levels.
// rank(y) = #{j < 255: code[j] < y}; q = rank or rank - 1, whichever is nearer in fp32, the lower index on a tie.
__device__ __forceinline__ int adam8_quant(const float* code, const float* tree, float x, float a) {
  const float y = a > 0.f ? x / a : 0.f;
  int k = 1;
#pragma unroll
  for (int l = 0; l < 8; ++l) k = 2 * k + (tree[k] < y ? 1 : 0);
  const int hi = k - 256, lo = hi > 0 ? hi - 1 : 0;
  return (y - code[lo] <= code[hi] - y) ? lo : hi;
}

template <bool EMA>
__global__ __launch_bounds__(256) void adamw8_kernel(float* p, const float* g, unsigned char* qm, unsigned char* qv, float* am, float* av, float* ema,
                                                     long long n, const float* code_m, const float* code_v, float lr, float b1, float b2, float eps,
                                                     float wd, float bc1, float bc2_sqrt, float gscale, float ema_w, const float* hyper) {
  __shared__ float s_cm[256], s_cv[256], s_tm[256], s_tv[256];
  {
    const int t = threadIdx.x;
    // tree node t (1..255) at level L = floor(log2 t), offset j = t - 2^L, is the sorted entry (2j + 1) * 2^(7 - L) - 1; node 0 is unused
    const int L = 31 - __clz(t | 1), idx = t ? (((2 * (t - (1 << L)) + 1) << (7 - L)) - 1) : 0;
    s_cm[t] = code_m[t]; s_cv[t] = code_v[t];
    s_tm[t] = code_m[idx]; s_tv[t] = code_v[idx];
  }
  __syncthreads();
  if (hyper) { lr = hyper[0]; bc1 = hyper[1]; bc2_sqrt = hyper[2]; gscale = hyper[3]; if constexpr (EMA) ema_w = hyper[4]; }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long nblk = (n + 255) / 256;
  for (long long blk = (long long)blockIdx.x * 4 + wave; blk < nblk; blk += (long long)gridDim.x * 4) {      // wave-uniform trip count
    const long long i = blk * 256 + lane * 4;
    const int cnt = i >= n ? 0 : (n - i >= 4 ? 4 : (int)(n - i));      // valid elements of this lane: 4, or fewer in the short last block
    const float a_m = am[blk], a_v = av[blk];
    float pp[4] = {0.f, 0.f, 0.f, 0.f}, gg[4] = {0.f, 0.f, 0.f, 0.f}, ee[4] = {0.f, 0.f, 0.f, 0.f};
    unsigned wm = 0, wv = 0;
    if (cnt == 4) {
      const float4 P = *(const float4*)(p + i), G = *(const float4*)(g + i);
      pp[0] = P.x; pp[1] = P.y; pp[2] = P.z; pp[3] = P.w;
      gg[0] = G.x * gscale; gg[1] = G.y * gscale; gg[2] = G.z * gscale; gg[3] = G.w * gscale;
      wm = *(const unsigned*)(qm + i); wv = *(const unsigned*)(qv + i);
      if constexpr (EMA) { const float4 E = *(const float4*)(ema + i); ee[0] = E.x; ee[1] = E.y; ee[2] = E.z; ee[3] = E.w; }
    } else {
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        if (k >= cnt) break;
        pp[k] = p[i + k]; gg[k] = g[i + k] * gscale;
        wm |= (unsigned)qm[i + k] << (8 * k); wv |= (unsigned)qv[i + k] << (8 * k);
        if constexpr (EMA) ee[k] = ema[i + k];
      }
    }
    float mm[4], vv[4], xm = 0.f, xv = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const bool ok = k < cnt;      // a lane's missing elements carry zeros: they leave the block maxima alone
      mm[k] = ok ? s_cm[(wm >> (8 * k)) & 255] * a_m : 0.f;
      vv[k] = ok ? s_cv[(wv >> (8 * k)) & 255] * a_v : 0.f;
      // adamw_kernel.inc's arithmetic, in its order, with the contractions adamw_kernel compiles to (-ffp-contract=fast) written out: the decay
      // 1 - lr * wd, b * moment + (1 - b) * gradient term and decay * p - step are one fma each, and no other product feeds a sum, so nothing is
      // left for the compiler to fuse one way in one instantiation and another way in the other; p moves by the unquantised new moments
      mm[k] = fmaf(b1, mm[k], (1.f - b1) * gg[k]);
      vv[k] = fmaf(b2, vv[k], (1.f - b2) * gg[k] * gg[k]);
      const float denom = sqrtf(vv[k]) / bc2_sqrt + eps;
      // (adamw_kernel's last partial quad goes through its scalar loop, where decay * p - step stayed a product and a difference: the lane that
      // holds such a quad here is the same lane of the same buffer, and does the same, so that from zero moments EVERY p' is e4t_adamw's.
      // The empty asm keeps the backend from fusing that product: -ffp-contract=fast is a property of the whole file.)
      const float decay = fmaf(-lr, wd, 1.f), upd = (lr / bc1) * mm[k] / denom;
      float prod = decay * pp[k];
      asm volatile("" : "+v"(prod));
      pp[k] = cnt == 4 ? fmaf(decay, pp[k], -upd) : prod - upd;
      xm = fmaxf(xm, fabsf(mm[k])); xv = fmaxf(xv, vv[k]);
    }
    xm = wave_max(xm); xv = wave_max(xv);
    wm = 0; wv = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      wm |= (unsigned)adam8_quant(s_cm, s_tm, mm[k], xm) << (8 * k);
      wv |= (unsigned)adam8_quant(s_cv, s_tv, vv[k], xv) << (8 * k);
    }
    if (cnt == 4) {
      *(float4*)(p + i) = make_float4(pp[0], pp[1], pp[2], pp[3]);
      *(unsigned*)(qm + i) = wm; *(unsigned*)(qv + i) = wv;
      if constexpr (EMA)
        *(float4*)(ema + i) = make_float4(ema_f(ee[0], pp[0], ema_w), ema_f(ee[1], pp[1], ema_w), ema_f(ee[2], pp[2], ema_w), ema_f(ee[3], pp[3], ema_w));
    } else {
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        if (k >= cnt) break;
        p[i + k] = pp[k];
        qm[i + k] = (unsigned char)(wm >> (8 * k)); qv[i + k] = (unsigned char)(wv >> (8 * k));
        if constexpr (EMA) ema[i + k] = ema_f(ee[k], pp[k], ema_w);
      }
    }
    if (lane == 0) { am[blk] = xm; av[blk] = xv; }
  }
}

// ---- AdamW of the E4T head's stacked first_linears weights with the gradient formed IN REGISTERS (round 6) ----
// The n = 129 weight gradients are rank-K products dW_i[r][c] = sum_k G[k][r] * Z[k][i*cols + c] (K = images of the step: the batch, or
// under data parallelism every rank's rows gathered; encoder.py:159-162): 845 MB of fp32 that the step used to write (batched GEMM), read
// back (AdamW) and clear (zero_grad).  Here a workgroup owns RB rows of one slot: a thread holds its 4 columns of the K x cols factor
// slice (bf16 -> fp32 registers, re-read from L2 by the cols / RB workgroups of the slot), the RB x K factor block of G sits in LDS
// and is read as broadcasts, and each element's gradient is a k-ordered fmaf chain in front of the same update arithmetic as
// adamw_kernel: 24 B of HBM traffic per parameter instead of 36, ~2 K FMAs per element on a kernel that stays HBM-bound.
template <int RB>
__global__ __launch_bounds__(320) void adamw_rank_kernel(float* p, float* m, float* v, const bf16_t* G, const bf16_t* Z, int rows, int cols, int K,
                                                         int ldg, long long ldz, float lr, float b1, float b2, float eps, float wd, float bc1,
                                                         float bc2_sqrt, float gscale, const float* hyper) {
  constexpr bool EMA = false;
  float* const ema = nullptr;
  float ema_w = 0.f;
#include "adamw_rank_kernel.inc"
}
template <int RB>
__global__ __launch_bounds__(320) void adamw_rank_ema_kernel(float* p, float* m, float* v, float* ema, const bf16_t* G, const bf16_t* Z, int rows, int cols,
                                                             int K, int ldg, long long ldz, float lr, float b1, float b2, float eps, float wd, float bc1,
                                                             float bc2_sqrt, float gscale, float ema_w, const float* hyper) {
  constexpr bool EMA = true;
#include "adamw_rank_kernel.inc"
}

// sum of squares of a flat fp32 buffer -> partial[blockIdx.x]
__global__ __launch_bounds__(256) void sumsq_kernel(const float* g, long long n, float* partial) {
  __shared__ float red[16];
  float s = 0.f;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) s += g[i] * g[i];
  s = block_sum(s, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// ---- host side ----
// The step's scalars as a launch carries them.  With hyper_dev the kernel reads lr, the bias corrections, the gradient scale (and the EMA weight)
// from device memory and the launch arguments are neutral; without it bc1 = 1 - beta1^step and bc2 = sqrt(1 - beta2^step).
struct StepArgs {
  float lr, bc1, bc2, gscale, ema_w;
  StepArgs(const float* hyper_dev, int step, float beta1, float beta2, float lr_, float grad_scale, float ema_w_)
      : lr(hyper_dev ? 0.f : lr_), bc1(hyper_dev ? 1.f : 1.f - powf(beta1, (float)step)), bc2(hyper_dev ? 1.f : sqrtf(1.f - powf(beta2, (float)step))),
        gscale(hyper_dev ? 1.f : grad_scale), ema_w(hyper_dev ? 0.f : ema_w_) {}
};

// e4t_adamw, e4t_adamw_hyper (need_hyper) and e4t_adamw_ema (with_ema): adamw_kernel, or adamw_ema_kernel over ema; 1024 elements per workgroup and trip
int adamw_flat(const char* name, bool need_hyper, bool with_ema, float* p, const float* g, float* m, float* v, float* ema, long long n, float lr, float beta1, float beta2,
               float eps, float weight_decay, int step, float grad_scale, float ema_w, const float* hyper_dev, hipStream_t s) {
  E4T_REQUIRE(p && g && m && v && (!with_ema || ema) && (!need_hyper || hyper_dev) && n > 0 && (hyper_dev || step >= 1), "%s: bad arguments", name);
  E4T_REQUIRE((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v | (uintptr_t)ema | (uintptr_t)hyper_dev) & 15) == 0, "%s: buffers must be 16-B aligned", name);
  const StepArgs a(hyper_dev, step, beta1, beta2, lr, grad_scale, ema_w);
  const dim3 grid(grid_for((n + 3) / 4, 4096));
  if (with_ema) {
    E4T_LOG_LAUNCH("adamw_ema_kernel|n%lld|%.0f|0", (long long)n, 36.0 * (double)n);
    hipLaunchKernelGGL(adamw_ema_kernel, grid, dim3(256), 0, s, p, g, m, v, ema, n, a.lr, beta1, beta2, eps, weight_decay, a.bc1, a.bc2, a.gscale, a.ema_w, hyper_dev);
    E4T_CHECK_LAUNCH("adamw_ema_kernel");
  } else {
    E4T_LOG_LAUNCH("adamw_kernel|n%lld|%.0f|0", (long long)n, 28.0 * (double)n);
    hipLaunchKernelGGL(adamw_kernel, grid, dim3(256), 0, s, p, g, m, v, n, a.lr, beta1, beta2, eps, weight_decay, a.bc1, a.bc2, a.gscale, hyper_dev);
    E4T_CHECK_LAUNCH("adamw_kernel");
  }
  return 0;
}

// e4t_adamw_rank and e4t_adamw_rank_ema (with_ema): adamw_rank_kernel, or adamw_rank_ema_kernel over ema
int adamw_rank(const char* name, bool with_ema, float* p, float* m, float* v, float* ema, const void* G, const void* Z, int n, int rows, int cols, int K, int ldg,
               long long ldz, float lr, float beta1, float beta2, float eps, float weight_decay, int step, float grad_scale, float ema_w, const float* hyper_dev,
               hipStream_t s) {
  E4T_REQUIRE(p && m && v && (!with_ema || ema) && G && Z && n > 0 && rows > 0 && cols > 0 && K > 0 && (hyper_dev || step >= 1), "%s: bad arguments", name);
  E4T_REQUIRE(cols % 4 == 0 && ldz % 4 == 0 && ldg >= rows && ldz >= (long long)n * cols, "%s: cols and the Z row stride must be multiples of 4", name);
  E4T_REQUIRE((((uintptr_t)p | (uintptr_t)m | (uintptr_t)v | (uintptr_t)ema) & 15) == 0 && ((uintptr_t)Z & 7) == 0 && ((uintptr_t)hyper_dev & 15) == 0,
              "%s: buffers must be 16-B (factors 8-B) aligned", name);
  const StepArgs a(hyper_dev, step, beta1, beta2, lr, grad_scale, ema_w);
  constexpr int RB = 8;
  const dim3 grid(cdiv(rows, RB), n), block(min(320, (cols / 4 + 63) / 64 * 64));
  const double flops = 2.0 * n * rows * (double)cols * K;      // algorithmic bytes: p, m, v (and ema) read and written; the factors are L2 traffic
  if (with_ema) {
    E4T_LOG_LAUNCH("adamw_rank_ema_kernel<%d>|n%d rows%d cols%d K%d|%.0f|%.0f", RB, n, rows, cols, K, 32.0 * n * rows * cols, flops);
    hipLaunchKernelGGL((adamw_rank_ema_kernel<RB>), grid, block, 0, s, p, m, v, ema, (const bf16_t*)G, (const bf16_t*)Z, rows, cols, K, ldg, ldz, a.lr, beta1,
                       beta2, eps, weight_decay, a.bc1, a.bc2, a.gscale, a.ema_w, hyper_dev);
    E4T_CHECK_LAUNCH("adamw_rank_ema_kernel");
  } else {
    E4T_LOG_LAUNCH("adamw_rank_kernel<%d>|n%d rows%d cols%d K%d|%.0f|%.0f", RB, n, rows, cols, K, 24.0 * n * rows * cols, flops);
    hipLaunchKernelGGL((adamw_rank_kernel<RB>), grid, block, 0, s, p, m, v, (const bf16_t*)G, (const bf16_t*)Z, rows, cols, K, ldg, ldz, a.lr, beta1, beta2,
                       eps, weight_decay, a.bc1, a.bc2, a.gscale, hyper_dev);
    E4T_CHECK_LAUNCH("adamw_rank_kernel");
  }
  return 0;
}
}  // namespace

extern "C" int e4t_adamw(float* p, const float* g, float* m, float* v, long long n, float lr, float beta1, float beta2, float eps, float weight_decay, int step,
                         float grad_scale, e4t_stream s) {
  return adamw_flat("adamw", false, false, p, g, m, v, nullptr, n, lr, beta1, beta2, eps, weight_decay, step, grad_scale, 0.f, nullptr, (hipStream_t)s);
}
extern "C" int e4t_adamw_hyper(float* p, const float* g, float* m, float* v, long long n, const float* hyper_dev, float beta1, float beta2, float eps, float weight_decay,
                               e4t_stream s) {
  return adamw_flat("adamw_hyper", true, false, p, g, m, v, nullptr, n, 0.f, beta1, beta2, eps, weight_decay, 0, 1.f, 0.f, hyper_dev, (hipStream_t)s);
}
extern "C" int e4t_adamw_ema(float* p, const float* g, float* m, float* v, float* ema, long long n, float lr, float beta1, float beta2, float eps, float weight_decay, int step,
                             float grad_scale, float ema_w, const float* hyper_dev, e4t_stream s) {
  return adamw_flat("adamw_ema", false, true, p, g, m, v, ema, n, lr, beta1, beta2, eps, weight_decay, step, grad_scale, ema_w, hyper_dev, (hipStream_t)s);
}
extern "C" int e4t_adamw_rank(float* p, float* m, float* v, const void* G, const void* Z, int n, int rows, int cols, int K, int ldg, long long ldz, float lr, float beta1,
                              float beta2, float eps, float weight_decay, int step, float grad_scale, const float* hyper_dev, e4t_stream s) {
  return adamw_rank("adamw_rank", false, p, m, v, nullptr, G, Z, n, rows, cols, K, ldg, ldz, lr, beta1, beta2, eps, weight_decay, step, grad_scale, 0.f, hyper_dev, (hipStream_t)s);
}
extern "C" int e4t_adamw_rank_ema(float* p, float* m, float* v, float* ema, const void* G, const void* Z, int n, int rows, int cols, int K, int ldg, long long ldz, float lr,
                                  float beta1, float beta2, float eps, float weight_decay, int step, float grad_scale, float ema_w, const float* hyper_dev, e4t_stream s) {
  return adamw_rank("adamw_rank_ema", true, p, m, v, ema, G, Z, n, rows, cols, K, ldg, ldz, lr, beta1, beta2, eps, weight_decay, step, grad_scale, ema_w, hyper_dev,
                    (hipStream_t)s);
}
extern "C" int e4t_adamw8(float* p, const float* g, void* qm, void* qv, float* absmax_m, float* absmax_v, float* ema, long long n, const float* code_m, const float* code_v,
                          float lr, float beta1, float beta2, float eps, float weight_decay, int step, float grad_scale, float ema_w, const float* hyper_dev, e4t_stream s) {
  E4T_REQUIRE(p && g && qm && qv && absmax_m && absmax_v && code_m && code_v && n > 0 && (hyper_dev || step >= 1), "adamw8: bad arguments");
  E4T_REQUIRE((((uintptr_t)p | (uintptr_t)g | (uintptr_t)ema | (uintptr_t)hyper_dev) & 15) == 0, "adamw8: p, g, ema and hyper_dev must be 16-B aligned");
  E4T_REQUIRE((((uintptr_t)qm | (uintptr_t)qv | (uintptr_t)absmax_m | (uintptr_t)absmax_v | (uintptr_t)code_m | (uintptr_t)code_v) & 3) == 0,
              "adamw8: codes, scales and codebooks must be 4-B aligned");
  const StepArgs a(hyper_dev, step, beta1, beta2, lr, grad_scale, ema_w);
  const int grid = grid_for((n + 3) / 4, 4096);      // 1024 elements (four blocks of 256, one per wave) per workgroup and trip, as adamw_kernel
  const double bytes = 16.0 * (double)n + 16.0 * (double)((n + 255) / 256) + (ema ? 8.0 * (double)n : 0.0);
  const char* name = ema ? "adamw8_ema_kernel" : "adamw8_kernel";
  E4T_LOG_LAUNCH("%s|n%lld grid%d|%.0f|0", name, (long long)n, grid, bytes);
  hipLaunchKernelGGL(ema ? adamw8_kernel<true> : adamw8_kernel<false>, dim3(grid), dim3(256), 0, (hipStream_t)s, p, g, (unsigned char*)qm, (unsigned char*)qv,
                     absmax_m, absmax_v, ema, n, code_m, code_v, a.lr, beta1, beta2, eps, weight_decay, a.bc1, a.bc2, a.gscale, a.ema_w, hyper_dev);
  E4T_CHECK_LAUNCH(name);
  return 0;
}
extern "C" int e4t_ema_update(float* ema, const float* p, long long n, float ema_w, const float* w_dev, e4t_stream s) {
  E4T_REQUIRE(ema && p && n > 0, "ema_update: bad arguments");
  E4T_REQUIRE((((uintptr_t)ema | (uintptr_t)p) & 15) == 0 && ((uintptr_t)w_dev & 3) == 0, "ema_update: buffers must be 16-B aligned");
  E4T_LOG_LAUNCH("ema_update_kernel|n%lld|%.0f|0", (long long)n, 12.0 * (double)n);
  hipLaunchKernelGGL(ema_update_kernel, dim3(grid_for((n + 3) / 4, 4096)), dim3(256), 0, (hipStream_t)s, ema, p, n, w_dev ? 0.f : ema_w, w_dev);
  E4T_CHECK_LAUNCH("ema_update_kernel");
  return 0;
}
extern "C" int e4t_sumsq_partial(const float* g, long long n, float* partial, int nblocks, e4t_stream s) {
  E4T_REQUIRE(g && partial && n > 0 && nblocks > 0, "sumsq_partial: bad arguments");
  hipLaunchKernelGGL(sumsq_kernel, dim3(nblocks), dim3(256), 0, (hipStream_t)s, g, n, partial);
  E4T_CHECK_LAUNCH("sumsq_kernel");
  return 0;
}
