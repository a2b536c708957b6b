// The sampling step on fp32 latents: classifier-free guidance fused with one update of a linear sampler (guided_step_kernel for the DDIM
// row alone, sampler_step_kernel for every sampler, with the img2img / inpainting blend and the guided variants as instances of one body),
// and the per-image statistics behind guidance rescale.  Coefficients live in device memory, so a captured step replays with new ones.
#include "common.h"
#include "../../include/e4t_hip.h"

// index of NCHW element i = (b, c, p) in pred, which may be in the UNet's NHWC output layout ([B][HW][C])
__device__ __forceinline__ long long pred_index(long long i, int C, int HW, int nhwc) {
  if (!nhwc) return i;
  const int p = (int)(i % HW), c = (int)((i / HW) % C), b = (int)(i / ((long long)HW * C));
  return ((long long)b * HW + p) * C + c;
}

// Classifier-free guidance + one linear scheduler update in a single pass (pipeline_stable_diffusion_e4t.py:209-214):
//   eps = cfg ? u + g*(c - u) : pred ;  out = c_sample*sample + c_pred*eps (+ c_noise*noise)
// coef = {g, c_sample, c_pred, c_noise} lives in device memory so a captured hipGraph of the step can be replayed with
// new coefficients.  pred may be given in the UNet's NHWC output layout ([B][HW][C]); sample / noise / out are NCHW.
__global__ __launch_bounds__(256) void guided_step_kernel(const float* __restrict__ pred, const float* __restrict__ sample, const float* __restrict__ noise,
                                                          float* __restrict__ out, const float* __restrict__ coef, int B, int C, int HW, int cfg, int nhwc) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long n = (long long)B * C * HW;
  if (i >= n) return;
  const float g = coef[0], cs = coef[1], cp = coef[2], cn = coef[3];
  const long long j = pred_index(i, C, HW, nhwc);
  float e = pred[j];
  if (cfg) {
    const float t = pred[j + n];
    e = e + g * (t - e);
  }
  float o = cs * sample[i] + cp * e;
  if (noise) o += cn * noise[i];
  out[i] = o;
}

// Per-image statistics of the guided value for guidance rescale (e4t_guidance_stats in the header): one workgroup of 1024
// threads per image, two passes over the image's N = C*HW values (means, then squared deviations from them; the second pass
// reads what the first left in L2).  A one-pass sum / sum of squares loses the deviation of an image whose mean is large
// against it.  An image's slab is the same N contiguous values in NCHW and NHWC, and a sum does not care which element is
// which, so both layouts walk the slab in storage order.  Every thread adds its strided elements in index order and block_sum
// combines in a fixed order: no atomics, the same bits on every call.  V = 4: 16-byte loads (N % 4 == 0, aligned pred).
__device__ __forceinline__ float guide_e0(float u, float t, float c, float g, float g_id, int branches) {
  if (branches == 3) return __fmaf_rn(g_id, c - t, __fmaf_rn(g, t - u, u));
  return u + g * (t - u);                                  // branches == 2: t is c; sampler_step_kernel's expression
}
template <int V>
__global__ __launch_bounds__(1024) void guidance_stats_kernel(const float* __restrict__ pred, const float* __restrict__ gp, float* __restrict__ gstat,
                                                              long long n, int N, int branches) {
  __shared__ float red[32];
  const float g = gp[0], g_id = gp[1], phi = gp[2];
  const float* u = pred + (long long)blockIdx.x * N;       // branch 0 of this image; branch r is at u + r*n
  const float* c = u + (branches - 1) * n;
  float vu[V], vt[V], vc[V];
  float se = 0.f, sc = 0.f;
  for (int i = threadIdx.x * V; i < N; i += 1024 * V) {
    if constexpr (V == 4) {
      *(float4*)vu = *(const float4*)(u + i);
      *(float4*)vt = *(const float4*)(u + n + i);
      *(float4*)vc = *(const float4*)(c + i);
    } else {
      vu[0] = u[i], vt[0] = u[n + i], vc[0] = c[i];
    }
#pragma unroll
    for (int v = 0; v < V; ++v) {
      se += guide_e0(vu[v], vt[v], vc[v], g, g_id, branches);
      sc += vc[v];
    }
  }
  const float me = block_sum(se, red) / (float)N, mc = block_sum(sc, red + 16) / (float)N;
  float qe = 0.f, qc = 0.f;
  for (int i = threadIdx.x * V; i < N; i += 1024 * V) {
    if constexpr (V == 4) {
      *(float4*)vu = *(const float4*)(u + i);
      *(float4*)vt = *(const float4*)(u + n + i);
      *(float4*)vc = *(const float4*)(c + i);
    } else {
      vu[0] = u[i], vt[0] = u[n + i], vc[0] = c[i];
    }
#pragma unroll
    for (int v = 0; v < V; ++v) {
      const float de = guide_e0(vu[v], vt[v], vc[v], g, g_id, branches) - me, dc = vc[v] - mc;
      qe = __fmaf_rn(de, de, qe);
      qc = __fmaf_rn(dc, dc, qc);
    }
  }
  qe = block_sum(qe, red);
  qc = block_sum(qc, red + 16);
  if (threadIdx.x == 0) {
    const float s_e = sqrtf(qe / (float)(N - 1)), s_c = sqrtf(qc / (float)(N - 1));
    const float ratio = s_c / s_e;
    const float f = (s_e == 0.f || !isfinite(ratio)) ? 1.f : (1.f - phi) + phi * ratio;
    float* o = gstat + (long long)blockIdx.x * E4T_GUIDE_STATS;
    o[0] = f, o[1] = s_c, o[2] = s_e, o[3] = me;
  }
}

// Guidance + one step of any linear sampler (DDIM, PLMS, LMS, Euler, Euler-ancestral, DPM-Solver++ 2M) in a single pass.
// The row contract is the header's (e4t_sampler_step).  Every thread owns one element index across x, out, hist, saved
// and x_in, so reading the old values before writing the new ones needs no synchronisation and x may alias out.
// Terms whose coefficient is 0 are skipped (uniform branch on a row value), which keeps a DDIM row's arithmetic exactly
// guided_step_kernel's: same expressions in the same order, so the same contraction.
// BLEND (e4t_sampler_step_edit): the finished o is mixed with the original latent re-noised to the level of the row's output,
// y = a_keep*x0 + s_keep*n0 with (a_keep, s_keep) = row[14], row[15], weighted by keep; both entry points are instances of
// this one body, and everything up to the mix is the same code, so the plain entry point's arithmetic cannot drift.
// GUIDED (e4t_sampler_step_guided): g comes from gp instead of row[0], a third branch [u | k | c] adds the identity term
// g_id*(c - k), and the guided value is scaled by the image's rescale factor gstat[b][0] (e4t_guidance_stats) when gstat is
// given.  With branches == 2 and no gstat the guidance line is the one the plain entry points run, so the bits are theirs.
template <bool BLEND, bool GUIDED>
__global__ __launch_bounds__(256) void sampler_step_kernel(const float* __restrict__ pred, const float* x, float* out, float* hist, float* saved,
                                                           const float* __restrict__ noise, float* x_in, const float* __restrict__ row,
                                                           const float* __restrict__ keep, const float* __restrict__ x0, const float* __restrict__ n0,
                                                           const float* __restrict__ gp, const float* __restrict__ gstat,
                                                           int B, int C, int HW, int K, int cfg, int nhwc, int x_in_copies,
                                                           int keep_per_image, int x0_per_image, int branches) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long n = (long long)B * C * HW;
  if (i >= n) return;
  const float g = GUIDED ? gp[0] : row[0], a_e = row[1], a_x = row[2], c_x = row[3], c_s = row[4], c_m = row[5], c_n = row[6], k_in = row[7];
  const int w = (int)row[8], save_x = row[9] != 0.f;
  const long long j = pred_index(i, C, HW, nhwc);
  float e = pred[j];
  if (cfg) {
    const float t = pred[j + n];
    if (GUIDED && branches == 3) e = __fmaf_rn(gp[1], pred[j + 2 * n] - t, __fmaf_rn(g, t - e, e));
    else e = e + g * (t - e);
  }
  if constexpr (GUIDED) {
    if (gstat) e *= gstat[(i / ((long long)C * HW)) * E4T_GUIDE_STATS];
  }
  const float xv = x[i];
  float m = a_e * e;
  if (a_x != 0.f) m = __fmaf_rn(a_x, xv, m);
  float o = c_x * xv + c_m * m;
  if (c_s != 0.f && saved) o = __fmaf_rn(c_s, saved[i], o);
  for (int k = 0; k < K; ++k) {
    const float ck = row[10 + k];
    if (ck != 0.f) o = __fmaf_rn(ck, hist[k * n + i], o);
  }
  if (noise && c_n != 0.f) o += c_n * noise[i];
  if (w >= 0 && w < K) hist[w * n + i] = m;
  if (save_x && saved) saved[i] = xv;
  if constexpr (BLEND) {
    const long long chw = (long long)C * HW;
    const float kp = keep[(keep_per_image ? (i / chw) * HW : 0) + i % HW];
    const float y = __fmaf_rn(row[15], n0[i], row[14] * x0[x0_per_image ? i : i % chw]);
    o = __fmaf_rn(kp, y, (1.f - kp) * o);
  }
  out[i] = o;
  if (x_in_copies > 0) {
    const float v = k_in * o;
    x_in[i] = v;
    if (x_in_copies > 1) x_in[n + i] = v;
    if (x_in_copies > 2) x_in[2 * n + i] = v;
  }
}

namespace {
// ---- host side of the three e4t_sampler_step* entries: the preconditions under the entry's name and in one order, then the launch ----
// guided: gp and branches are the entry's (e4t_sampler_step_guided); need_blend: keep, x0 and n0 are required (e4t_sampler_step_edit), otherwise
// all of them or none (the plain entry has no such arguments and passes nulls and zeros); max_copies: how many copies of the next UNet input
// the entry may write.  BLEND is instantiated when keep is given, GUIDED when gp is.
int sampler_step(const char* name, const char* launch_name, bool guided, bool need_blend, int max_copies, const float* pred, const float* x, float* out, float* hist,
                 float* saved, const float* noise, float* x_in, const float* row, const float* gp, const float* gstat, const float* keep, const float* x0, const float* n0,
                 int B, int C, int HW, int K, int cfg, int branches, int pred_nhwc, int x_in_copies, int keep_per_image, int x0_per_image, hipStream_t s) {
  E4T_REQUIRE(pred && x && out && row && (!guided || gp) && B > 0 && C > 0 && HW > 0, "%s: bad arguments", name);
  if (guided) E4T_REQUIRE(branches == 2 || branches == 3, "%s: branches = %d (2: [u | c], 3: [u | k | c])", name, branches);
  if (need_blend) E4T_REQUIRE(keep && x0 && n0, "%s: keep, x0 and n0 are required", name);
  E4T_REQUIRE((keep && x0 && n0) || (!keep && !x0 && !n0), "%s: keep, x0 and n0 are given together or not at all", name);
  E4T_REQUIRE((keep_per_image == 0 || keep_per_image == 1) && (x0_per_image == 0 || x0_per_image == 1), "%s: keep_per_image = %d, x0_per_image = %d (0 or 1)",
              name, keep_per_image, x0_per_image);
  E4T_REQUIRE(K >= 0 && K <= E4T_SAMPLER_MAX_HIST && (K == 0 || hist), "%s: K = %d history slots (0..%d, hist required when K > 0)", name, K, E4T_SAMPLER_MAX_HIST);
  E4T_REQUIRE(x_in_copies >= 0 && x_in_copies <= max_copies && (x_in_copies == 0 || x_in), "%s: x_in_copies = %d (0..%d, x_in required when > 0)", name, x_in_copies, max_copies);
  auto* kernel = keep ? (gp ? sampler_step_kernel<true, true> : sampler_step_kernel<true, false>)
                      : (gp ? sampler_step_kernel<false, true> : sampler_step_kernel<false, false>);
  hipLaunchKernelGGL(kernel, dim3((unsigned)cdivl((long long)B * C * HW, 256)), dim3(256), 0, s, pred, x, out, hist, saved, noise, x_in, row, keep, x0, n0, gp,
                     gstat, B, C, HW, K, cfg, pred_nhwc, x_in_copies, keep_per_image, x0_per_image, branches);
  E4T_CHECK_LAUNCH(launch_name);
  return 0;
}
}  // namespace

extern "C" int e4t_guided_step(const float* pred, const float* sample, const float* noise, float* out, const float* coef, int B, int C, int HW, int cfg, int pred_nhwc,
                               e4t_stream s) {
  E4T_REQUIRE(pred && sample && out && coef && B > 0 && C > 0 && HW > 0, "guided_step: bad arguments");
  const long long n = (long long)B * C * HW;
  hipLaunchKernelGGL(guided_step_kernel, dim3((unsigned)cdivl(n, 256)), dim3(256), 0, (hipStream_t)s, pred, sample, noise, out, coef, B, C, HW, cfg, pred_nhwc);
  E4T_CHECK_LAUNCH("guided_step_kernel");
  return 0;
}
extern "C" int e4t_guidance_stats(const float* pred, const float* gp, float* gstat, int B, int C, int HW, int branches, int pred_nhwc, e4t_stream s) {
  E4T_REQUIRE(pred, "guidance_stats: pred is null");
  E4T_REQUIRE(gp, "guidance_stats: gp is null");
  E4T_REQUIRE(gstat, "guidance_stats: gstat is null");
  E4T_REQUIRE(branches == 2 || branches == 3, "guidance_stats: branches = %d (2: [u | c], 3: [u | k | c])", branches);
  E4T_REQUIRE(B > 0 && C > 0 && HW > 0 && (long long)C * HW <= 0x7fffffffLL, "guidance_stats: B = %d, C = %d, HW = %d", B, C, HW);
  E4T_REQUIRE((long long)C * HW >= 2, "guidance_stats: N = C*HW = %lld values per image (an unbiased deviation needs N >= 2)", (long long)C * HW);
  (void)pred_nhwc;                                         // storage order: see the kernel
  const int N = C * HW;
  const long long n = (long long)B * N;
  const bool vec = N % 4 == 0 && ((uintptr_t)pred & 15) == 0;
  hipLaunchKernelGGL(vec ? guidance_stats_kernel<4> : guidance_stats_kernel<1>, dim3(B), dim3(1024), 0, (hipStream_t)s, pred, gp, gstat, n, N, branches);
  E4T_CHECK_LAUNCH("guidance_stats_kernel");
  return 0;
}
extern "C" int e4t_sampler_step(const float* pred, const float* x, float* out, float* hist, float* saved, const float* noise, float* x_in, const float* row, int B, int C,
                                int HW, int K, int cfg, int pred_nhwc, int x_in_copies, e4t_stream s) {
  return sampler_step("sampler_step", "sampler_step_kernel", false, false, 2, pred, x, out, hist, saved, noise, x_in, row, nullptr, nullptr, nullptr, nullptr, nullptr,
                      B, C, HW, K, cfg, 2, pred_nhwc, x_in_copies, 0, 0, (hipStream_t)s);
}
extern "C" int e4t_sampler_step_edit(const float* pred, const float* x, float* out, float* hist, float* saved, const float* noise, float* x_in, const float* row,
                                     const float* keep, const float* x0, const float* n0, int B, int C, int HW, int K, int cfg, int pred_nhwc, int x_in_copies,
                                     int keep_per_image, int x0_per_image, e4t_stream s) {
  return sampler_step("sampler_step_edit", "sampler_step_edit_kernel", false, true, 2, pred, x, out, hist, saved, noise, x_in, row, nullptr, nullptr, keep, x0, n0,
                      B, C, HW, K, cfg, 2, pred_nhwc, x_in_copies, keep_per_image, x0_per_image, (hipStream_t)s);
}
extern "C" int e4t_sampler_step_guided(const float* pred, const float* x, float* out, float* hist, float* saved, const float* noise, float* x_in, const float* row,
                                       const float* gp, const float* gstat, const float* keep, const float* x0, const float* n0, int B, int C, int HW, int K, int branches,
                                       int pred_nhwc, int x_in_copies, int keep_per_image, int x0_per_image, e4t_stream s) {
  return sampler_step("sampler_step_guided", "sampler_step_guided_kernel", true, false, 3, pred, x, out, hist, saved, noise, x_in, row, gp, gstat, keep, x0, n0,
                      B, C, HW, K, 1, branches, pred_nhwc, x_in_copies, keep_per_image, x0_per_image, (hipStream_t)s);
}
