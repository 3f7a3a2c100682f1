// The dense exact-f32 phase path of MUR, k <= 128: the Itakura-Saito divergence (NMFX_IS), per-entry weights Omega >= 0
// (nmfx_upload_weights) under the Euclidean, KL and IS losses, and the beta-divergence (nmfx_set_beta, NMFX_BETA) with or
// without weights.  One phase kernel, one pair of update kernels and one host scaffold; the six paths differ in a per-entry
// policy (Entry) and in the closed form of the update.
//
// The skeleton.  Both phases are ONE kernel template with the roles of the two factors swapped (phase_kernel).  Per 16-wide
// stage of the contracted dimension a wave loads its V slice (and, where the policy asks, the Omega slice) in the register
// layout of the f32 MFMA's output, forms the tile of T = W H in that layout, lets the policy turn each (v, om, T) into a
// numerator and a denominator entry in registers and feeds each into a second MFMA product: two accumulators per output
// tile.  The quotients never leave the registers.  The W phase also sums the objective terms of the pair it starts from
// (f32 per stage, f64 across stages).  Slabs [num | den] of the split contracted dimension are summed in slab order by the
// update kernels: no atomics, two runs are bit-identical.  Fold-in (nmfx_foldin_run, W fixed) runs the H phase alone and lets
// IT sum the objective of the pair it starts from: one pass over V per step (the end of this file).
//
// The policies.  q = T + 1e-9, W' = the new W, H likewise with W' and lam_h.
//   IsEntry          num = v / q^2             den = 1 / q       term  v / q - log(v / q) - 1
//                    W <- W o sqrt( (num H^T) / (den H^T + lam_w) ),  a zero denominator gives 0
//                    (the MM rule with exponent 1/2 of Fevotte & Idier 2011: it cannot increase the objective at lam = 0)
//   WtEntry<EU>      num = om v                den = om T        term  om (v - T)^2, the sum halved
//                    W <- W o (num H^T) / (den H^T + lam_w W + 1e-9)
//   WtEntry<KL>      num = om v / (T + 1e-9)   den = om          term  om [v log(v / T) - v + T]
//                    A = W o (num H^T),  B = den H^T,  W <- 2 A / (B + sqrt(B^2 + 4 lam_w A)),  0 where B = 0
//   WtEntry<IS>      num = om v / q^2          den = om / q      term  om [v / q - log(v / q) - 1];   the update of IsEntry
//   BetaEntry<WT>    den = om q^(beta-1)       num = om v q^(beta-1) / q      (om = 1 without weights)
//                    term  om d_beta(v | q),  d_beta = (v^beta + (beta-1) q^beta - beta v q^(beta-1)) / (beta (beta-1)),
//                          v log(v / q) - v + q at beta = 1,  v / q - log(v / q) - 1 at beta = 0
//                    W <- W o ( (num H^T) / (den H^T + lam_w) )^gamma,  a zero denominator gives 0
//                    gamma = 1 / (2 - beta) for beta < 1,  1 for 1 <= beta <= 2,  1 / (beta - 1) for beta > 2
//                    (the MM rule of Fevotte & Idier 2011: no half-step increases the objective at lam = 0)
//
// Padding and live cells.  Padded cells of V and Omega are 0.
//   IsEntry selects nothing: a padded v is 0, so num = 0; den = 1e9 there meets a zero factor entry on one side or lands in
//   a padded output, which the update kernels overwrite with 0 without reading the sums.  The objective term is taken only
//   where v > 0 (v = 0 is zero padding: IS data is strictly positive).
//   WtEntry and BetaEntry<true>: a cell is live where om > 0; om = 0 is padding or an unknown cell, where V is not part of
//   any sum.  BetaEntry<false>: for beta > 0 a zero of V is data, so a padded cell cannot be told by v = 0 -- and it has
//   q = 1e-9, i.e. a large q^(beta-1) for beta < 1 and an objective term (1e-9)^beta / beta; a cell is live where row < m
//   and column < n.  Elsewhere num, den and the term are SELECTED to 0 (live ? ... : 0), never multiplied to 0: what the
//   other branch holds there (1 / 1e-9 from a zero T, 0 / 0, the logarithm of 0, whatever bits V has) is discarded, so no
//   0 * 1e9 or 0 * inf product is ever formed and every loss gives exact zeros.  A padded factor component multiplies finite
//   num / den by its zero entries (exact 0) and the update kernels write 0 there without reading the sums.  A row / column
//   of the kept index that is all padding or carries no weight receives num = den = 0 and its closed form gives 0:
//   Euclidean 0 / (lam w + 1e-9), KL B = 0 -> 0, the power forms den + lam = 0 -> 0 and w (0 / lam)^gamma = 0 otherwise.
//
// Automatic relevance determination (nmfx_set_ard) rides on BetaEntry: the phase kernel is untouched, the update
// kernels add pen[c] = phi / lambda_c of the entry's component c to the denominator in place of the scalar lam, and two small
// kernels recompute lambda_c = (|w_c|_1 + |h_c|_1 + b) / c after every H update (ard_sums_kernel, ard_finish_kernel).
//
// The power.  q^(beta-1) through the hardware's log2 / exp2 carries a relative error of about |beta-1| |ln q| times that of
// the logarithm (1e-5 at q = 1e-9): powf, which keeps the logarithm's low part, is within an ulp for every q and is what
// both BetaEntry and the general-gamma update use.  gamma = 1 and 1/2 are a plain quotient and sqrtf.
//
// The beta objective.  The three-term form divided by beta (beta-1) amplifies f32 rounding by 1 / |beta (beta-1)| on top of
// the 1 / |d| of any divergence near a good fit.  With r = v / q rounded once and t = log r the term is
//     q^beta ( expm1(beta t) - beta (r - 1) ) / (beta (beta-1)),       r - 1 = expm1(t) of that same r
// which has no 1 / beta blow-up (expm1(beta t) / beta is smooth through beta = 0), gives q^beta / beta at v = 0 for beta > 0
// (t = -inf: expm1 = -1, r - 1 = -1, nothing undefined) and reuses q^(beta-1).  Both halves see the SAME rounded r, so the
// rounding of r moves the term by 2 ulp / |t| of itself; an exact (v - q) / q beside the logarithm of the rounded r would
// cost ulp / t^2 (CPU emulation).  beta exactly 0 and exactly 1 take the limit forms, r - 1 - t and
// q (r t - (r - 1)), on the same r.
#include "nmfx_internal.h"
#include "kernels_small.h"

#define MFMA(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)

// --------------------------------------------------------------------------
// The per-entry policies.  OMEGA: the kernel loads the Omega slice (w is 1 otherwise).  SELECT: num and den are selected
// to 0 where the cell is not live; the objective term always is.  FOLDIN_ONLY: the policy exists for fold-in alone (see
// PlainEntry).  live(v, w, inside): inside = row < m and column < n.
// entry<OBJ>(args, v, w, T, nu, de, term): num, den and -- OBJ only -- the objective term of one cell.  OBJ_SCALE: what the
// block's objective sum is multiplied by.  Args: the policy's run-time parameters, a kernel argument passed by value.
// --------------------------------------------------------------------------
struct NoArgs {};

struct IsEntry {
    using Args = NoArgs;
    static constexpr bool OMEGA = false, SELECT = false, FOLDIN_ONLY = false;
    static constexpr double OBJ_SCALE = 1.0;
    static __device__ __forceinline__ bool live(float v, float, bool) { return v > 0.f; }
    template <bool OBJ>
    static __device__ __forceinline__ void entry(const Args&, float v, float, float T, float& nu, float& de, float& term) {
        const float iq = 1.f / (T + 1e-9f);
        const float rq = v * iq;
        if (OBJ) term = (rq - 1.f) - logf(rq);
        nu = rq * iq;
        de = iq;
    }
};

template <int LOSS>
struct WtEntry {
    using Args = NoArgs;
    static constexpr bool OMEGA = true, SELECT = true, FOLDIN_ONLY = false;
    static constexpr double OBJ_SCALE = LOSS == NMFX_EU ? 0.5 : 1.0;
    static __device__ __forceinline__ bool live(float, float w, bool) { return w > 0.f; }
    template <bool OBJ>
    static __device__ __forceinline__ void entry(const Args&, float v, float w, float T, float& nu, float& de, float& term) {
        if (LOSS == NMFX_EU) {
            const float d = v - T;
            if (OBJ) term = w * (d * d);
            nu = w * v;
            de = w * T;
        } else if (LOSS == NMFX_KL) {
            if (OBJ) {
                float tl = v * logf(v / T);
                tl = (tl != tl || tl == __builtin_inff()) ? 0.f : tl;
                term = w * ((tl - v) + T);
            }
            nu = w * (v / (T + 1e-9f));
            de = w;
        } else {
            const float iq = 1.f / (T + 1e-9f);
            const float rq = v * iq;
            if (OBJ) term = w * ((rq - 1.f) - logf(rq));
            nu = w * (rq * iq);
            de = w * iq;
        }
    }
};

// The Omega-free Euclidean and KL policies of fold-in (nmfx_foldin_run): the per-entry functions of WtEntry<EU | KL> with
// om = 1, no Omega stream, live cells by index (a zero of V is data).  FOLDIN_ONLY: instantiated in the two combinations
// fold-in launches alone, the H phase with objective and the objective-only pass (launch_phase).
template <int LOSS>
struct PlainEntry {
    using Args = NoArgs;
    static constexpr bool OMEGA = false, SELECT = true, FOLDIN_ONLY = true;
    static constexpr double OBJ_SCALE = LOSS == NMFX_EU ? 0.5 : 1.0;
    static __device__ __forceinline__ bool live(float, float, bool inside) { return inside; }
    template <bool OBJ>
    static __device__ __forceinline__ void entry(const Args&, float v, float, float T, float& nu, float& de, float& term) {
        if (LOSS == NMFX_EU) {
            const float d = v - T;
            if (OBJ) term = d * d;
            nu = v;
            de = T;
        } else {
            if (OBJ) {
                float tl = v * logf(v / T);
                tl = (tl != tl || tl == __builtin_inff()) ? 0.f : tl;
                term = (tl - v) + T;
            }
            nu = v / (T + 1e-9f);
            de = 1.f;
        }
    }
};

// beta and what the host derives from it (in f64, then rounded)
struct BetaArgs {
    float beta, bm1;       // beta, beta - 1
    float inv_bb1;         // 1 / (beta (beta - 1));  unused at beta = 0, 1
    int form;              // objective: 0 general, 1 the beta = 0 limit, 2 the beta = 1 limit
};

template <bool WT>
struct BetaEntry {
    using Args = BetaArgs;
    static constexpr bool OMEGA = WT, SELECT = true, FOLDIN_ONLY = false;
    static constexpr double OBJ_SCALE = 1.0;
    static __device__ __forceinline__ bool live(float, float w, bool inside) { return WT ? w > 0.f : inside; }
    template <bool OBJ>
    static __device__ __forceinline__ void entry(const Args& ba, float v, float w, float T, float& nu, float& de, float& term) {
        const float qv = T + 1e-9f;
        const float iq = 1.f / qv;
        de = powf(qv, ba.bm1);
        nu = (v * de) * iq;
        if (OBJ) {
            const float rq = v * iq, tt = logf(rq);     // (v = 0, beta > 0: rq = 0, tt = -inf, expm1 = -1)
            if (ba.form == 1) term = (rq - 1.f) - tt;
            else if (ba.form == 2) term = qv * ((v > 0.f ? rq * tt : 0.f) - (rq - 1.f));
            else term = ((de * qv) * (expm1f(ba.beta * tt) - ba.beta * (rq - 1.f))) * ba.inv_bb1;
            if (WT) term *= w;
        }
        if (WT) { nu *= w; de *= w; }
    }
};

// --------------------------------------------------------------------------
// One phase.  "Kept" index u: a column of V (H phase) / a row of V (W phase); "contracted" index s: the other one.
//   F  = the factor along s:  F[s][c] = W[s][c] (H phase) / H[c][s] (W phase)
//   P  = the panel of the factor along u, in LDS: P[c][i] = H[c][u0 + i] (H phase) / W[u0 + i][c] (W phase)
// Block = 16 NE kept indices x the contracted range of split blockIdx.y, its 16-wide stages dealt to the 4 waves.
// Stage:
//   T tile e  = F(16 x KP) . P(KP x 16)              -> lane (x, q) reg r = (W H) at (s0 + 4q + r, u0 + 16e + x)
//   num, den per entry by Entry (V and Omega loaded in that same layout)
//   nacc[j][e] += F(4 stage rows, tile j)^T . num(4 stage rows, tile e),  dacc likewise with den     for the 4 groups r
// Output slab of split sr: [num | den], each [KP][np] (H phase) / [mp][KP] (W phase).
// m, n: the logical shape of V (the live cells of BetaEntry<false>).
// --------------------------------------------------------------------------
template <typename Entry, int KP, int NE, bool WPH, bool UPD, bool OBJ>
__global__ __launch_bounds__(256) void phase_kernel(
    const float* __restrict__ V, const float* __restrict__ Om, int64_t ldv, const float* __restrict__ W,
    const float* __restrict__ H, float* __restrict__ part, double* __restrict__ objpart, int64_t np, int64_t mp,
    int64_t m, int64_t n, typename Entry::Args ea, const int* __restrict__ flag)
{
    if (*flag) return;
    constexpr int JT = KP / 16;
    constexpr int LDP = 16 * NE + 4;
    constexpr bool OMEGA = Entry::OMEGA;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, x = lane & 15, q = lane >> 4;
    const int SR = gridDim.y, sr = blockIdx.y;
    const int64_t k0 = (int64_t)blockIdx.x * 16 * NE;
    const int64_t n16 = (WPH ? np : mp) / 16;
    const int64_t u0 = n16 * sr / SR, u1 = n16 * (sr + 1) / SR;
    const int64_t t0 = u0 + (u1 - u0) * wave / 4, t1 = u0 + (u1 - u0) * (wave + 1) / 4;
    const int64_t kept_end = WPH ? m : n, contr_end = WPH ? n : m;

    for (int i = tid; i < KP * 16 * NE; i += 256) {
        if (WPH) { const int r = i / KP, c = i % KP; lds[c * LDP + r] = W[(k0 + r) * KP + c]; }
        else { const int c = i / (16 * NE), r = i % (16 * NE); lds[c * LDP + r] = H[(int64_t)c * np + k0 + r]; }
    }
    __syncthreads();

    f32x4 nacc[UPD ? JT : 1][UPD ? NE : 1], dacc[UPD ? JT : 1][UPD ? NE : 1];
    if (UPD) {
#pragma unroll
        for (int j = 0; j < JT; ++j)
#pragma unroll
            for (int e = 0; e < NE; ++e) { nacc[j][e] = (f32x4){0.f, 0.f, 0.f, 0.f}; dacc[j][e] = (f32x4){0.f, 0.f, 0.f, 0.f}; }
    }
    double osum = 0.0;

    for (int64_t t = t0; t < t1; ++t) {
        const int64_t s0 = t * 16;
        float fa[JT][4], fb[4][UPD ? JT : 1], vv[NE][4], om[OMEGA ? NE : 1][4];
        if (WPH) {
#pragma unroll
            for (int u = 0; u < JT; ++u)
#pragma unroll
                for (int s = 0; s < 4; ++s) fa[u][s] = H[(int64_t)(16 * u + 4 * q + s) * np + s0 + x];
            if (UPD) {
#pragma unroll
                for (int j = 0; j < JT; ++j) {
                    const float4 f = *reinterpret_cast<const float4*>(H + (int64_t)(16 * j + x) * np + s0 + 4 * q);
                    fb[0][j] = f.x; fb[1][j] = f.y; fb[2][j] = f.z; fb[3][j] = f.w;
                }
            }
#pragma unroll
            for (int e = 0; e < NE; ++e) {
                const int64_t at = (k0 + 16 * e + x) * ldv + s0 + 4 * q;
                const float4 v = *reinterpret_cast<const float4*>(V + at);
                vv[e][0] = v.x; vv[e][1] = v.y; vv[e][2] = v.z; vv[e][3] = v.w;
                if (OMEGA) {
                    const float4 o = *reinterpret_cast<const float4*>(Om + at);
                    om[e][0] = o.x; om[e][1] = o.y; om[e][2] = o.z; om[e][3] = o.w;
                }
            }
        } else {
#pragma unroll
            for (int u = 0; u < JT; ++u) {
                const float4 f = *reinterpret_cast<const float4*>(W + (s0 + x) * KP + 16 * u + 4 * q);
                fa[u][0] = f.x; fa[u][1] = f.y; fa[u][2] = f.z; fa[u][3] = f.w;
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
#pragma unroll
                for (int e = 0; e < NE; ++e) {
                    const int64_t at = (s0 + 4 * q + r) * ldv + k0 + 16 * e + x;
                    vv[e][r] = V[at];
                    if (OMEGA) om[e][r] = Om[at];
                }
                if (UPD) {
#pragma unroll
                    for (int j = 0; j < JT; ++j) fb[r][j] = W[(s0 + 4 * q + r) * KP + 16 * j + x];
                }
            }
        }
        f32x4 pe[NE];
#pragma unroll
        for (int e = 0; e < NE; ++e) pe[e] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int u = 0; u < JT; ++u)
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const float* prow = lds + (16 * u + 4 * q + s) * LDP + x;
#pragma unroll
                for (int e = 0; e < NE; ++e) pe[e] = MFMA(fa[u][s], prow[16 * e], pe[e]);
            }
        // per entry: vv <- num, pe <- den (header, "Padding and live cells")
        float part_obj = 0.f;
#pragma unroll
        for (int e = 0; e < NE; ++e)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float v = vv[e][r], w = OMEGA ? om[OMEGA ? e : 0][r] : 1.f;
                const bool live = Entry::live(v, w, k0 + 16 * e + x < kept_end && s0 + 4 * q + r < contr_end);
                float nu, de, term = 0.f;
                Entry::template entry<OBJ>(ea, v, w, pe[e][r], nu, de, term);
                if (OBJ) part_obj += live ? term : 0.f;
                vv[e][r] = Entry::SELECT && !live ? 0.f : nu;
                pe[e][r] = Entry::SELECT && !live ? 0.f : de;
            }
        if (OBJ) osum += (double)part_obj;
        if (UPD) {
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int j = 0; j < JT; ++j)
#pragma unroll
                    for (int e = 0; e < NE; ++e) {
                        nacc[j][e] = MFMA(fb[r][j], vv[e][r], nacc[j][e]);
                        dacc[j][e] = MFMA(fb[r][j], pe[e][r], dacc[j][e]);
                    }
        }
    }
    __syncthreads();                                            // the panel is no longer needed

    if (UPD) {
        // fixed-order cross-wave sum, then store (each lane owns its LDS words)
        f32x4* red = reinterpret_cast<f32x4*>(lds);             // [2][JT * NE][64]
        const int64_t count = (int64_t)KP * (WPH ? mp : np);
        float* slab = part + (int64_t)sr * 2 * count;
#pragma unroll 1
        for (int w = 0; w < 4; ++w) {
            if (wave == w) {
#pragma unroll
                for (int h = 0; h < 2; ++h)
#pragma unroll
                    for (int j = 0; j < JT; ++j)
#pragma unroll
                        for (int e = 0; e < NE; ++e) {
                            const f32x4 mine = h ? dacc[j][e] : nacc[j][e];
                            const int slot = ((h * JT + j) * NE + e) * 64 + lane;
                            if (w == 0) red[slot] = mine;
                            else if (w < 3) red[slot] += mine;
                            else {
                                const f32x4 tt = red[slot] + mine;
                                float* out = slab + h * count;
                                if (WPH) {
                                    *reinterpret_cast<f32x4*>(out + (k0 + 16 * e + x) * KP + 16 * j + 4 * q) = tt;
                                } else {
#pragma unroll
                                    for (int g = 0; g < 4; ++g) out[(int64_t)(16 * j + 4 * q + g) * np + k0 + 16 * e + x] = tt[g];
                                }
                            }
                        }
            }
            __syncthreads();
        }
    }
    if (OBJ) {
        if (Entry::OBJ_SCALE != 1.0) osum *= Entry::OBJ_SCALE;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) osum += __shfl_down(osum, off, 64);
        double* ored = reinterpret_cast<double*>(lds);
        if (lane == 0) ored[wave] = osum;
        __syncthreads();
        if (tid == 0) objpart[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = ((ored[0] + ored[1]) + ored[2]) + ored[3];
    }
}

// The closed forms on f = the old factor entry, a / d = the summed numerator / denominator.  CF_ONE, CF_HALF and CF_POW are
// f (a / (d + lam))^gamma with gamma = 1, 1/2 and any other gamma; d + lam = 0 gives 0.
enum { CF_EU, CF_KL, CF_ONE, CF_HALF, CF_POW };

__device__ __forceinline__ float closed_form(int form, float gamma, float f, float a, float d, float lam) {
    if (form == CF_EU) return (f * a) / ((d + lam * f) + 1e-9f);
    if (form == CF_KL) {
        const float A = f * a;
        return d > 0.f ? (2.f * A) / (d + sqrtf(d * d + (4.f * lam) * A)) : 0.f;
    }
    d += lam;
    if (!(d > 0.f)) return 0.f;
    const float r = a / d;
    return f * (form == CF_ONE ? r : form == CF_HALF ? sqrtf(r) : powf(r, gamma));
}

// W_new from the slabs' numerators / denominators, summed in slab order.  pen (ARD; nullptr otherwise): the per-component
// penalty [kp] that takes the place of lam
__global__ __launch_bounds__(256) void phase_w_update_kernel(
    const float* __restrict__ part, int splits, int64_t count, int kp, int k, int form, float gamma,
    const float* __restrict__ Wold, float lam, const float* __restrict__ pen, float* __restrict__ Wnew, const int* __restrict__ flag)
{
    if (*flag) return;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    if ((int)(i % kp) >= k) { Wnew[i] = 0.f; return; }       // padded factors stay zero: 0/0 must stay out
    float a = part[i], d = part[count + i];
    for (int p = 1; p < splits; ++p) { a += part[(int64_t)(2 * p) * count + i]; d += part[(int64_t)(2 * p + 1) * count + i]; }
    Wnew[i] = closed_form(form, gamma, Wold[i], a, d, pen ? pen[i % kp] : lam);
}

// H_new after the objective bookkeeping / convergence test (same protocol as MUR-KL).  pen as above; ardobj (ARD; nullptr
// otherwise): the penalty of the pair whose objective xf64[0] holds, added to it in f64 before it is recorded
__global__ __launch_bounds__(256) void phase_h_update_kernel(
    const float* __restrict__ part, int splits, const double* __restrict__ xf64, float* __restrict__ H, int64_t np, int kp,
    int k, int form, float gamma, float lam, const float* __restrict__ pen, const double* __restrict__ ardobj, long long j,
    long long min_iter, double tol1, double tol2, DevState* __restrict__ st, double* __restrict__ obj_hist)
{
    if (st->flag) return;
    const int rule = nmfx_record_objective(st, obj_hist, ardobj ? xf64[0] + ardobj[0] : xf64[0], j, min_iter, tol1, tol2,
                                           blockIdx.x == 0 && threadIdx.x == 0);
    if (rule) return;
    const int64_t count = (int64_t)kp * np;
    const int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i >= count) return;
    if (i / np >= k) return;                                 // padded factor rows stay zero
    float4 a = *reinterpret_cast<const float4*>(part + i), d = *reinterpret_cast<const float4*>(part + count + i);
    for (int p = 1; p < splits; ++p) {
        const float4 ta = *reinterpret_cast<const float4*>(part + (int64_t)(2 * p) * count + i);
        const float4 td = *reinterpret_cast<const float4*>(part + (int64_t)(2 * p + 1) * count + i);
        a.x += ta.x; a.y += ta.y; a.z += ta.z; a.w += ta.w;
        d.x += td.x; d.y += td.y; d.z += td.z; d.w += td.w;
    }
    const float4 h = *reinterpret_cast<const float4*>(H + i);
    const float l = pen ? pen[i / np] : lam;                 // (np is a multiple of 4: the four entries share a row)
    float4 o;
    o.x = closed_form(form, gamma, h.x, a.x, d.x, l);
    o.y = closed_form(form, gamma, h.y, a.y, d.y, l);
    o.z = closed_form(form, gamma, h.z, a.z, d.z, l);
    o.w = closed_form(form, gamma, h.w, a.w, d.w, l);
    *reinterpret_cast<float4*>(H + i) = o;
}

// --------------------------------------------------------------------------
// ARD: the relevances lambda_c = (|w_c|_1 + |h_c|_1 + b) / c of the components c < k, in f64 from the f32 factors, in two stages
// with a fixed order of additions (no atomics: two runs are bit-identical).
//   ard_sums_kernel    blocks [0, nwb): ARD_WROWS rows of W [mp][kp] each, read as whole rows of float4 (thread t of a pass = the
//                      t-th float4 of a contiguous 4 KiB); a thread keeps four f64 column sums over its rows, thread cg < kp / 4
//                      then adds the row lanes' sums in lane order -> sums[block][kp]
//                      blocks [nwb, nwb + k nhc): row c of H [kp][np], columns [ARD_HCOLS chunk, ...), float4 per thread; f64
//                      per thread, shuffle tree, the four waves in order -> sums[nwb + chunk][c]
//   ard_finish_kernel  one block; thread c < k adds the W partials in block order, then the H partials in chunk order;
//                      lam[c] = (sw + sh + b) / cc, pen[c] = (float)(phi / lam[c]); thread 0 adds the terms 1 + log lam[c]
//                      in component order -> lam[kp] = phi cc Sum.  Padded components (c >= k) get lam = pen = 0 and no term.
// flag: the run's stop flag (a stopped run keeps the relevances of the pair it stopped at), or nullptr.
constexpr int ARD_WROWS = 128;       // mp is a multiple of 128
constexpr int ARD_HCOLS = 2048;

__global__ __launch_bounds__(256) void ard_sums_kernel(
    const float* __restrict__ W, const float* __restrict__ H, int64_t np, int kp, int k, int nwb, int nhc,
    double* __restrict__ sums, const int* __restrict__ flag)
{
    if (flag && *flag) return;
    __shared__ double sh[256 * 4];
    const int tid = threadIdx.x;
    if ((int)blockIdx.x < nwb) {
        const int c4 = kp / 4, lanes = 256 / c4;             // float4 per row (4 .. 32), row lanes (64 .. 8)
        const int cg = tid % c4, rl = tid / c4;
        const float* base = W + (int64_t)blockIdx.x * ARD_WROWS * kp + 4 * cg;
        double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
        for (int r = rl; r < ARD_WROWS; r += lanes) {
            const float4 f = *reinterpret_cast<const float4*>(base + (int64_t)r * kp);
            s0 += (double)f.x; s1 += (double)f.y; s2 += (double)f.z; s3 += (double)f.w;
        }
        sh[tid * 4 + 0] = s0; sh[tid * 4 + 1] = s1; sh[tid * 4 + 2] = s2; sh[tid * 4 + 3] = s3;
        __syncthreads();
        if (tid < c4) {
            double t0 = 0.0, t1 = 0.0, t2 = 0.0, t3 = 0.0;
            for (int l = 0; l < lanes; ++l) {
                const double* p = sh + (l * c4 + tid) * 4;
                t0 += p[0]; t1 += p[1]; t2 += p[2]; t3 += p[3];
            }
            double* out = sums + (int64_t)blockIdx.x * kp + 4 * tid;
            out[0] = t0; out[1] = t1; out[2] = t2; out[3] = t3;
        }
    } else {
        const int hb = (int)blockIdx.x - nwb, c = hb / nhc, chunk = hb % nhc;      // c < k by the grid
        const int64_t c0 = (int64_t)chunk * ARD_HCOLS, c1 = c0 + ARD_HCOLS < np ? c0 + ARD_HCOLS : np;
        const float* row = H + (int64_t)c * np;
        double s = 0.0;
        for (int64_t at = c0 + 4 * tid; at < c1; at += 1024) {
            const float4 f = *reinterpret_cast<const float4*>(row + at);
            s += (((double)f.x + (double)f.y) + (double)f.z) + (double)f.w;
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
        if ((tid & 63) == 0) sh[tid >> 6] = s;
        __syncthreads();
        if (tid == 0) sums[(int64_t)(nwb + chunk) * kp + c] = ((sh[0] + sh[1]) + sh[2]) + sh[3];
    }
}

__global__ __launch_bounds__(128) void ard_finish_kernel(
    const double* __restrict__ sums, int nwb, int nhc, int kp, int k, double phi, double b, double cc,
    double* __restrict__ lam, float* __restrict__ pen, const int* __restrict__ flag)
{
    if (flag && *flag) return;
    __shared__ double term[128];
    const int t = threadIdx.x;
    if (t < kp) {
        double l = 0.0, tm = 0.0;
        float p = 0.f;
        if (t < k) {
            double sw = 0.0, sh = 0.0;
            for (int i = 0; i < nwb; ++i) sw += sums[(int64_t)i * kp + t];
            for (int i = 0; i < nhc; ++i) sh += sums[(int64_t)(nwb + i) * kp + t];
            l = ((sw + sh) + b) / cc;
            p = (float)(phi / l);
            tm = 1.0 + log(l);
        }
        lam[t] = l; pen[t] = p; term[t] = tm;
    }
    __syncthreads();
    if (t == 0) {
        double s = 0.0;
        for (int i = 0; i < k; ++i) s += term[i];
        lam[kp] = (phi * cc) * s;
    }
}

// the closing step of an ARD run: obj[j] = the objective of the last pair + its penalty, and the stop rule
__global__ void ard_finalize_kernel(const double* __restrict__ xf64, const double* __restrict__ ardobj, long long j, long long min_iter,
                                    double tol1, double tol2, DevState* __restrict__ st, double* __restrict__ obj_hist)
{
    if (st->flag) return;
    nmfx_record_objective(st, obj_hist, xf64[0] + ardobj[0], j, min_iter, tol1, tol2, threadIdx.x == 0);
}

// --------------------------------------------------------------------------
// The three families of paths: what words their errors and names their profiling scopes
struct PhasePath { const char* who; const char* wscope; const char* hscope; };
static const PhasePath PATH_IS = {"IS", "is_wphase", "is_hphase"};
static const PhasePath PATH_WT = {"weighted MUR", "wt_wphase", "wt_hphase"};
static const PhasePath PATH_BETA = {"MUR-beta", "beta_wphase", "beta_hphase"};
static const PhasePath PATH_PLAIN = {"fold-in", "plain_objective", "plain_hphase"};      // (PlainEntry: fold-in alone)
static const PhasePath& phase_path(const nmfx_engine* E, int distance) {
    return distance == NMFX_BETA ? PATH_BETA : E->Om ? PATH_WT : distance == NMFX_IS ? PATH_IS : PATH_PLAIN;
}

// Splits of the contracted dimension: enough blocks for two per CU, at least 8 stages (2 per wave) each
static int phase_splits(const nmfx_engine* E, int64_t blocks_x, int64_t stages) {
    const int64_t want = (2 * (int64_t)E->ncu + blocks_x - 1) / blocks_x;
    return (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(want, 16), stages / 8));
}
static int phase_ne(int kp) { return kp == 128 ? 2 : 4; }
static int phase_wsplits(const nmfx_engine* E) { return phase_splits(E, E->mp / (16 * phase_ne(E->kp)), E->np / 16); }
static int phase_hsplits(const nmfx_engine* E) { return phase_splits(E, E->np / (16 * phase_ne(E->kp)), E->mp / 16); }

// slabs of both phases share one buffer: the W update has consumed the W phase's before the H phase writes its own
static int phase_ensure(nmfx_engine* E) {
    const int64_t need = 2 * std::max<int64_t>((int64_t)phase_wsplits(E) * E->mp * E->kp, (int64_t)phase_hsplits(E) * E->kp * E->np);
    if (E->phase_part && E->phase_part_cap >= need) return NMFX_OK;
    if (E->phase_part) { NMFX_HIP(hipStreamSynchronize(E->stream)); NMFX_HIP(hipFree(E->phase_part)); E->phase_part = nullptr; E->phase_part_cap = 0; }
    NMFX_HIP(hipMalloc(reinterpret_cast<void**>(&E->phase_part), (size_t)need * sizeof(float)));
    E->phase_part_cap = need;
    return NMFX_OK;
}

static BetaArgs beta_args(const nmfx_engine* E) {
    const double b = E->beta;
    BetaArgs a;
    a.beta = (float)b;
    a.bm1 = (float)(b - 1.0);
    a.form = b == 0.0 ? 1 : b == 1.0 ? 2 : 0;
    a.inv_bb1 = a.form ? 0.f : (float)(1.0 / (b * (b - 1.0)));
    return a;
}
static double beta_gamma(double b) { return b < 1.0 ? 1.0 / (2.0 - b) : b <= 2.0 ? 1.0 : 1.0 / (b - 1.0); }

// the closed form of a distance's update (plain and weighted IS: the exponent 1/2)
static int update_form(const nmfx_engine* E, int distance, float* gamma) {
    const double g = distance == NMFX_BETA ? beta_gamma(E->beta) : 0.5;
    *gamma = (float)g;
    if (distance == NMFX_EU) return CF_EU;
    if (distance == NMFX_KL) return CF_KL;
    return g == 1.0 ? CF_ONE : g == 0.5 ? CF_HALF : CF_POW;
}

template <typename Entry, int KP, int NE>
static int launch_phase(nmfx_engine* E, const PhasePath& P, const typename Entry::Args& ea, bool wph, bool upd, bool obj, const float* W) {
    const int splits = wph ? phase_wsplits(E) : phase_hsplits(E);
    dim3 grid((unsigned)((wph ? E->mp : E->np) / (16 * NE)), (unsigned)splits), block(256);
    const size_t panel = (size_t)KP * (16 * NE + 4) * sizeof(float);
    const size_t red = (size_t)2 * (KP / 16) * NE * 64 * sizeof(f32x4);
    const size_t shm = std::max(panel, red);
    { int rc_ = nmfx_need_v(E); if (rc_) return rc_; }
    // One objective partial per block, on either grid.  Both grids fit the buffer nmfx_create sized: a phase grid has
    // blocks_x * splits <= blocks_x * ceil(2 ncu / blocks_x) < 2 ncu + blocks_x blocks (phase_splits), blocks_x is at most
    // mp / 32 or np / 32, and obj_part_cap is 2 (max(mp, np) / 64 + 64) + 2 ncu or more.  Checked all the same.
    if (obj) {
        if ((int64_t)grid.x * grid.y > E->obj_part_cap) { E->err = std::string(P.who) + ": objective partials exceed their buffer"; return NMFX_E_ARG; }
        E->obj_count = (int64_t)grid.x * grid.y;
    }
#define NMFX_PHASELAUNCH(WP, UP, OB) \
    hipLaunchKernelGGL((phase_kernel<Entry, KP, NE, WP, UP, OB>), grid, block, shm, E->stream, E->V, E->Om, E->np, W, E->H, \
                       E->phase_part, E->obj_part, E->np, E->mp, E->m, E->n, ea, &E->state->flag)
    // the four combinations: W phase (with the objective), objective only, H phase, H phase with the objective (fold-in)
    if constexpr (Entry::FOLDIN_ONLY) {
        if (wph && !upd && obj) NMFX_PHASELAUNCH(true, false, true);
        else if (!wph && upd && obj) NMFX_PHASELAUNCH(false, true, true);
        else { E->err = std::string(P.who) + ": this policy runs fold-in alone"; return NMFX_E_ARG; }
    } else {
        if (wph) { if (upd) NMFX_PHASELAUNCH(true, true, true); else NMFX_PHASELAUNCH(true, false, true); }
        else if (obj) NMFX_PHASELAUNCH(false, true, true);
        else NMFX_PHASELAUNCH(false, true, false);
    }
#undef NMFX_PHASELAUNCH
    NMFX_HIP(hipGetLastError());
    return NMFX_OK;
}

template <typename Entry>
static int phase_kp(nmfx_engine* E, const PhasePath& P, const typename Entry::Args& ea, bool wph, bool upd, bool obj, const float* W) {
    switch (E->kp) {
        case 16: return launch_phase<Entry, 16, 4>(E, P, ea, wph, upd, obj, W);
        case 32: return launch_phase<Entry, 32, 4>(E, P, ea, wph, upd, obj, W);
        case 64: return launch_phase<Entry, 64, 4>(E, P, ea, wph, upd, obj, W);
        case 128: return launch_phase<Entry, 128, 2>(E, P, ea, wph, upd, obj, W);
    }
    E->err = std::string(P.who) + ": unsupported padded rank";
    return NMFX_E_ARG;
}

// the policy of a call: NMFX_BETA with or without weights, any other distance with weights, NMFX_IS without; fold-in
// alone (foldin) also runs the Euclidean and KL losses without weights.  obj: the objective is summed (every W-side pass)
static int phase(nmfx_engine* E, int distance, bool wph, bool upd, const float* W, bool foldin = false) {
    const bool obj = wph || foldin;
    if (distance == NMFX_BETA) {
        if (!E->beta_set) { E->err = "MUR-beta: no beta set (nmfx_set_beta)"; return NMFX_E_STATE; }
        const BetaArgs ba = beta_args(E);
        return E->Om ? phase_kp<BetaEntry<true>>(E, PATH_BETA, ba, wph, upd, obj, W) : phase_kp<BetaEntry<false>>(E, PATH_BETA, ba, wph, upd, obj, W);
    }
    if (E->Om) {
        switch (distance) {
            case NMFX_EU: return phase_kp<WtEntry<NMFX_EU>>(E, PATH_WT, NoArgs{}, wph, upd, obj, W);
            case NMFX_KL: return phase_kp<WtEntry<NMFX_KL>>(E, PATH_WT, NoArgs{}, wph, upd, obj, W);
            case NMFX_IS: return phase_kp<WtEntry<NMFX_IS>>(E, PATH_WT, NoArgs{}, wph, upd, obj, W);
        }
    } else if (distance == NMFX_IS) {
        return phase_kp<IsEntry>(E, PATH_IS, NoArgs{}, wph, upd, obj, W);
    } else if (foldin && distance == NMFX_EU) {
        return phase_kp<PlainEntry<NMFX_EU>>(E, PATH_PLAIN, NoArgs{}, wph, upd, obj, W);
    } else if (foldin && distance == NMFX_KL) {
        return phase_kp<PlainEntry<NMFX_KL>>(E, PATH_PLAIN, NoArgs{}, wph, upd, obj, W);
    }
    E->err = "Unknown distance type.";
    return NMFX_E_ARG;
}

int nmfx_mur_dense_phase_a(nmfx_engine* E, int distance, double lambda_w, int64_t j) {
    const PhasePath& P = phase_path(E, distance);
    const float* Wold = E->W[j & 1];
    float* Wnew = E->W[(j + 1) & 1];
    int rc;
    if ((rc = phase_ensure(E))) return rc;
    { ProfScope ps(E, P.wscope);
      if ((rc = phase(E, distance, true, true, Wold))) return rc; }
    { ProfScope ps(E, "w_update");
      const int64_t count = E->mp * E->kp;
      float gamma;
      const int form = update_form(E, distance, &gamma);
      hipLaunchKernelGGL(phase_w_update_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, E->stream, E->phase_part,
                         phase_wsplits(E), count, E->kp, E->k, form, gamma, Wold, (float)lambda_w,
                         E->ard ? (const float*)E->ard_pen : (const float*)nullptr, Wnew, &E->state->flag);
      NMFX_HIP(hipGetLastError()); }
    { ProfScope ps(E, P.hscope);
      if ((rc = phase(E, distance, false, true, Wnew))) return rc; }
    return nmfx_launch_obj_reduce(E, E->obj_count);
}

int nmfx_mur_dense_phase_b(nmfx_engine* E, int distance, double lambda_h, int64_t min_iter, double tol1, double tol2, int64_t j) {
    { ProfScope ps(E, "h_update");
      const int64_t n4 = ((int64_t)E->kp * E->np) / 4;
      float gamma;
      const int form = update_form(E, distance, &gamma);
      hipLaunchKernelGGL(phase_h_update_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, E->stream, E->phase_part,
                         phase_hsplits(E), E->xf64, E->H, E->np, E->kp, E->k, form, gamma, (float)lambda_h,
                         E->ard ? (const float*)E->ard_pen : (const float*)nullptr,
                         E->ard ? (const double*)(E->ard_lam + E->kp) : (const double*)nullptr, (long long)j,
                         (long long)min_iter, tol1, tol2, E->state, E->obj_hist);
      NMFX_HIP(hipGetLastError()); }
    // ARD: the relevances of the pair this iteration leaves, (W_{j+1}, H_{j+1}); skipped where the stop rule has just fired
    if (E->ard) return nmfx_ard_relevance(E, E->W[(j + 1) & 1], true);
    return NMFX_OK;
}

// ---- ARD (nmfx_set_ard) ---------------------------------------------------
static int ard_wblocks(const nmfx_engine* E) { return (int)(E->mp / ARD_WROWS); }
static int ard_hchunks(const nmfx_engine* E) { return (int)((E->np + ARD_HCOLS - 1) / ARD_HCOLS); }

// one zeroed ARD buffer, unless it exists: a call that failed half way is completed by the next one
template <typename T>
static int ard_buffer(nmfx_engine* E, T** p, size_t count) {
    if (*p) return NMFX_OK;
    T* buf = nullptr;
    NMFX_HIP(hipMalloc(reinterpret_cast<void**>(&buf), count * sizeof(T)));
    const hipError_t e = hipMemsetAsync(buf, 0, count * sizeof(T), E->stream);
    if (e != hipSuccess) { (void)hipFree(buf); E->err = std::string("ard_buffer: ") + hipGetErrorString(e); return NMFX_E_HIP; }
    *p = buf;
    return NMFX_OK;
}

// all three buffers or an error: nmfx_set_ard turns ARD on only behind NMFX_OK
int nmfx_ard_alloc(nmfx_engine* E) {
    int rc;
    if ((rc = ard_buffer(E, &E->ard_sums, (size_t)(ard_wblocks(E) + ard_hchunks(E)) * E->kp))) return rc;
    if ((rc = ard_buffer(E, &E->ard_lam, (size_t)E->kp + 1))) return rc;
    return ard_buffer(E, &E->ard_pen, (size_t)E->kp);
}

// lambda, phi / lambda and the penalty of (W, E->H); c = m + n + a + 1
int nmfx_ard_relevance(nmfx_engine* E, const float* W, bool honour_stop) {
    ProfScope ps(E, "ard_relevance");
    const int nwb = ard_wblocks(E), nhc = ard_hchunks(E);
    const int* flag = honour_stop ? &E->state->flag : nullptr;
    hipLaunchKernelGGL(ard_sums_kernel, dim3((unsigned)(nwb + E->k * nhc)), dim3(256), 0, E->stream, W, (const float*)E->H, E->np,
                       E->kp, E->k, nwb, nhc, E->ard_sums, flag);
    NMFX_HIP(hipGetLastError());
    hipLaunchKernelGGL(ard_finish_kernel, dim3(1), dim3(128), 0, E->stream, (const double*)E->ard_sums, nwb, nhc, E->kp, E->k,
                       E->ard_phi, E->ard_b, (double)E->m + (double)E->n + E->ard_a + 1.0, E->ard_lam, E->ard_pen, flag);
    NMFX_HIP(hipGetLastError());
    return NMFX_OK;
}

int nmfx_ard_finish_b(nmfx_engine* E, int64_t min_iter, double tol1, double tol2, int64_t j) {
    ProfScope ps(E, "small");
    hipLaunchKernelGGL(ard_finalize_kernel, dim3(1), dim3(64), 0, E->stream, (const double*)E->xf64, (const double*)(E->ard_lam + E->kp),
                       (long long)j, (long long)min_iter, tol1, tol2, E->state, E->obj_hist);
    NMFX_HIP(hipGetLastError());
    return NMFX_OK;
}

int nmfx_mur_dense_finish_a(nmfx_engine* E, int distance, int64_t j) {
    int rc;
    { ProfScope ps(E, "objective");
      if ((rc = phase(E, distance, true, false, E->W[j & 1]))) return rc; }
    return nmfx_launch_obj_reduce(E, E->obj_count);
}

// ---- fold-in (nmfx_foldin_run) -----------------------------
// One step with W fixed: the H phase, which here also sums the objective of the pair (W, H_j) it starts from; the reduce;
// phase_h_update_kernel, which records that objective, applies the stop rule and then updates H.  One pass over V.
int nmfx_foldin_step(nmfx_engine* E, int distance, double lambda_h, int64_t min_iter, double tol1, double tol2, int64_t j, const float* W) {
    const PhasePath& P = phase_path(E, distance);
    int rc;
    if ((rc = phase_ensure(E))) return rc;
    { ProfScope ps(E, P.hscope);
      if ((rc = phase(E, distance, false, true, W, true))) return rc; }
    if ((rc = nmfx_launch_obj_reduce(E, E->obj_count))) return rc;
    return nmfx_mur_dense_phase_b(E, distance, lambda_h, min_iter, tol1, tol2, j);
}

// the objective of the last pair: the objective-only pass
int nmfx_foldin_finish_a(nmfx_engine* E, int distance, const float* W) {
    int rc;
    { ProfScope ps(E, "objective");
      if ((rc = phase(E, distance, true, false, W, true))) return rc; }
    return nmfx_launch_obj_reduce(E, E->obj_count);
}

// (nmfx_create: forces this translation unit's code object onto the device under the library's start-up lock)
int nmfx_preload_phase() { hipFuncAttributes a; return hipFuncGetAttributes(&a, reinterpret_cast<const void*>(phase_w_update_kernel)) == hipSuccess ? 0 : -1; }
