// MUR on sparse V (nmfx_create_csr / nmfx_upload_csr): both losses, one GPU.  (HALS and its fold-in on the same handle, then the
// MUR fold-in: the last four sections.)
//
// Layout.  Both factors are row-major along their long dimension: W [m][kp] (double buffered, E->W) and H^T [n][kp]
// (nmfx_sparse::Ht), kp in {4, 8, 16, 32, 64, 128, 256}.  V is held twice: CSR (the W phase walks rows of V and gathers
// rows of H^T) and CSC (the H phase walks columns of V and gathers rows of the new W).  Both phases are one kernel
// template with the roles swapped (sp_phase_kernel).
//
// One wave owns one "unit": a whole row, or a piece of at most SP_CHUNK non-zeros of a longer one.  Inside the wave,
// groups of G = kp / 4 lanes each take one non-zero at a time (float4 of the gathered row per lane), NG = 64 / G
// non-zeros per step, four steps' gathers in flight.  Per non-zero: wh = <own row, gathered row> in f64 (products of f32
// are exact in f64), then the objective term of the pair the W phase starts from, then Sum x h (Euclidean) or
// Sum x / (wh + 1e-9) h (KL).  The groups' sums are combined by a fixed xor butterfly.  A whole row finishes with the
// update epilogue of nmf/mur.py:20-49; a piece stores its sum into a slab, and a second launch (sp_fixup_kernel) adds a
// long row's pieces in piece order and applies the same epilogue.
//
// No atomics: k x k Grams and column sums are per-slab f64 partials summed in slab order (sp_stats_kernel /
// sp_stats_reduce_kernel), objective partials are one f64 per block summed in block order (sp_objective_kernel).
// Unit -> wave assignment is a fixed stride over the unit list built at upload, so two runs are bit-identical.
//
// Objective (nmf/utils.py:18-33) over all m n entries, from the non-zeros plus k x k / k-sized terms:
//   Euclidean  1/2 [ ||X||^2 - 2 Sum_nz x wh + <W^T W, H H^T> ]      (||X||^2 in f64 at upload, Grams in f64)
//   KL         Sum_nz [x log(x / wh) - x] + Sum_c colsum(W)_c rowsum(H)_c     (inf / nan log terms -> 0, as the reference)
//
// Masked handles (nmfx_set_masked): the stored entries are the observed set M and nothing else is part of the fit.  The
// phase kernels (MASKED = true) sum a second float4 per lane in the same pass, the denominator of the masked update:
//   Euclidean  a = Sum_M x h,  d = Sum_M (float) wh h      out = w a / (d + lam w + 1e-9)
//   KL         a = Sum_M x / (wh + 1e-9) h,  d = Sum_M h   out = 2 w a / (d + sqrt(d^2 + 4 lam w a)),  d = 0 -> 0
// Pieces store [a | d] (slab [pieces][2 kp]).  The objective is summed per observed entry in f64 (Euclidean 1/2 (x - wh)^2,
// KL x log(x / wh) - x + wh); there are no Grams, column sums nor ||X||^2 terms, and no sp_stats_kernel passes.
//
// Itakura-Saito on masked handles (template parameter IS, masked instantiations only; q = wh + 1e-9 in f64):
//   a = Sum_M x / q^2 h,  d = Sum_M (1 / q) h     out = w sqrt(a / (d + lam)),  d + lam = 0 -> 0
// and the objective Sum_M [x / q - log(x / q) - 1] per observed entry in f64.  The Euclidean and KL instantiations are the
// ones they were: IS is a trailing parameter that defaults to false and only adds `if constexpr` branches.
#include "kernels_small.h"
#include <algorithm>
#include <cmath>
#include <cstring>
#include <type_traits>

#define SP_CHUNK 256          // non-zeros per unit: longer rows are split into pieces
#define SP_WAVES 8            // waves per block of the phase kernels

struct SpUnit { long long beg; int row; int len; int slot; int pad; };   // slot -1: a whole row; else the piece's slab row
struct SpLong { int row; int slot0; int npieces; int unit0; };          // a row split into pieces [slot0, slot0 + npieces): the units [unit0, unit0 + npieces)

struct SpSide {               // one orientation of V: 0 = CSR (W phase), 1 = CSC (H phase)
    int64_t rows = 0;
    int32_t* idx = nullptr;   // [nnz] column (CSR) / row (CSC) of each non-zero
    float* val = nullptr;     // [nnz]
    SpUnit* units = nullptr; int64_t nunits = 0;
    SpLong* longs = nullptr; int64_t nlong = 0;
    float* slab = nullptr;    // [pieces][kp] ([pieces][2 kp] on a masked handle)
    double* slab64 = nullptr; // [pieces][kp] in f64: the pieces' right-hand sides of the sparse HALS H phase (allocated at first use)
    int64_t npieces = 0;
    int nblk = 1;             // blocks of the phase kernel (a fixed stride over the units)
};

struct nmfx_sparse {
    int64_t nnz = 0;
    double x2 = 0.0;          // ||X||^2 of the stored (f32) values, in f64
    SpSide side[2];
    float* Ht = nullptr;      // H^T [n][kp]
    double* g64[2] = {nullptr, nullptr};   // [0] W^T W, [1] H H^T  [kp][kp]
    float* gf[2] = {nullptr, nullptr};     // ... in f32 (the Euclidean epilogues)
    double* cs64[2] = {nullptr, nullptr};  // [0] column sums of W, [1] row sums of H  [kp]
    float* csf[2] = {nullptr, nullptr};
    double* stat_part = nullptr;           // [slabs][kp * kp + kp]
    double* obj_part = nullptr;            // [blocks]
    int obj_cap = 0;
    double* hals_part = nullptr;           // sparse HALS: [blocks of the H phase | blocks of its fix-up] partials of Sum_nz x wh (allocated at first use)
    float* hals_r32 = nullptr;             // sparse HALS at kp = 256: the right-hand sides the sweep reads, [max(m, n)][kp] (allocated at first use)
    double* hals_r64 = nullptr;            // ... and the H phase's in f64, [n][kp]: the cross term reads them unrounded
    bool masked = false;      // the stored entries are the observed set (nmfx_set_masked)
    int32_t* foldin_sweeps = nullptr;      // HALS fold-in: [n] sweeps each column of H took (allocated at first use)
    bool foldin_done = false;              // ... of a solve that has run since nmfx_set_factors
    int32_t* mur_foldin_iters = nullptr;   // MUR fold-in: [n] steps each column of H took (allocated at first use)
    bool mur_foldin_done = false;          // ... of a run since nmfx_set_factors (a flag of its own: neither getter reads the other's counts)
};

// ---------------------------------------------------------------------------------------------------------------------
// device code
// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float4 sp_xor4(float4 a, int off) {
    return make_float4(__shfl_xor(a.x, off, 64), __shfl_xor(a.y, off, 64), __shfl_xor(a.z, off, 64), __shfl_xor(a.w, off, 64));
}
__device__ __forceinline__ float4 sp_add4(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
__device__ __forceinline__ float sp_comp(float4 a, int c) { return c == 0 ? a.x : c == 1 ? a.y : c == 2 ? a.z : a.w; }

// Sum over the NG groups of a wave (lanes with equal position in their group); every lane ends with the same bits.
template <int G>
__device__ __forceinline__ float4 sp_sum_groups(float4 a) {
#pragma unroll
    for (int off = G; off < 64; off <<= 1) a = sp_add4(a, sp_xor4(a, off));
    return a;
}

// The update epilogue of one owned row (every lane of the wave takes part; group 0 writes).  sp_epilogue_value returns the
// new row, this lane's four components (every group holds the same bits); sp_epilogue writes it.
//   Euclidean  out = w a / (w G + lam w + 1e-9)                         (nmf/mur.py:30, 45: (WH)H^T = W (H H^T))
//   KL         out = 2 w a / (s + sqrt(s^2 + 4 lam w a)),  s = sums     (nmf/mur.py:25-27, 40-42)
// Components c >= k (the zero padding) are written as 0.
template <int KP, bool KL>
__device__ __forceinline__ float4 sp_epilogue_value(float4 w4, float4 a4, const float* __restrict__ Gsrc, const float* __restrict__ S,
                                                    float lam, int k, int lig, int grp)
{
    constexpr int G = KP / 4, NG = 64 / G;
    float4 o;
    if constexpr (KL) {
        const float4 s4 = *reinterpret_cast<const float4*>(S + lig * 4);
        float c;
        c = w4.x * a4.x; o.x = 2.f * c / (s4.x + sqrtf(s4.x * s4.x + 4.f * lam * c));
        c = w4.y * a4.y; o.y = 2.f * c / (s4.y + sqrtf(s4.y * s4.y + 4.f * lam * c));
        c = w4.z * a4.z; o.z = 2.f * c / (s4.z + sqrtf(s4.z * s4.z + 4.f * lam * c));
        c = w4.w * a4.w; o.w = 2.f * c / (s4.w + sqrtf(s4.w * s4.w + 4.f * lam * c));
    } else {
        // d = w G for this lane's four components; the groups split the rows of G (l4 = grp, grp + NG, ...), w_l comes
        // from lane l / 4 (group 0; every group holds the same owned row)
        float4 d = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int l4 = grp; l4 < G; l4 += NG) {
            const float wl[4] = {__shfl(w4.x, l4, 64), __shfl(w4.y, l4, 64), __shfl(w4.z, l4, 64), __shfl(w4.w, l4, 64)};
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const float4 g = *reinterpret_cast<const float4*>(Gsrc + (4 * l4 + t) * KP + lig * 4);
                d.x = fmaf(wl[t], g.x, d.x); d.y = fmaf(wl[t], g.y, d.y);
                d.z = fmaf(wl[t], g.z, d.z); d.w = fmaf(wl[t], g.w, d.w);
            }
        }
        d = sp_sum_groups<G>(d);
        o.x = w4.x * a4.x / (d.x + lam * w4.x + 1e-9f);
        o.y = w4.y * a4.y / (d.y + lam * w4.y + 1e-9f);
        o.z = w4.z * a4.z / (d.z + lam * w4.z + 1e-9f);
        o.w = w4.w * a4.w / (d.w + lam * w4.w + 1e-9f);
    }
    const int c0 = lig * 4;
    if (c0 + 0 >= k) o.x = 0.f;
    if (c0 + 1 >= k) o.y = 0.f;
    if (c0 + 2 >= k) o.z = 0.f;
    if (c0 + 3 >= k) o.w = 0.f;
    return o;
}
template <int KP, bool KL>
__device__ __forceinline__ void sp_epilogue(float4 w4, float4 a4, const float* __restrict__ Gsrc, const float* __restrict__ S,
                                            float lam, int k, float* __restrict__ out_row, int lig, int grp)
{
    const float4 o = sp_epilogue_value<KP, KL>(w4, a4, Gsrc, S, lam, k, lig, grp);
    if (grp == 0) *reinterpret_cast<float4*>(out_row + lig * 4) = o;
}

// The update epilogue of one owned row on a masked handle, with the denominator d summed by the pass (no Gram, no sums):
//   Euclidean  out = w a / (d + lam w + 1e-9)
//   KL         out = 2 w a / (d + sqrt(d^2 + 4 lam w a)), and 0 where d = 0 (no observed entry: 0 / 0 is defined as 0)
template <bool KL, bool IS = false>
__device__ __forceinline__ float4 sp_epilogue_masked_value(float4 w4, float4 a4, float4 d4, float lam, int k, int lig)
{
    float4 o;
    if constexpr (IS) {
        float d;
        d = d4.x + lam; o.x = d > 0.f ? w4.x * sqrtf(a4.x / d) : 0.f;
        d = d4.y + lam; o.y = d > 0.f ? w4.y * sqrtf(a4.y / d) : 0.f;
        d = d4.z + lam; o.z = d > 0.f ? w4.z * sqrtf(a4.z / d) : 0.f;
        d = d4.w + lam; o.w = d > 0.f ? w4.w * sqrtf(a4.w / d) : 0.f;
    } else if constexpr (KL) {
        float c;
        c = w4.x * a4.x; o.x = d4.x > 0.f ? 2.f * c / (d4.x + sqrtf(d4.x * d4.x + 4.f * lam * c)) : 0.f;
        c = w4.y * a4.y; o.y = d4.y > 0.f ? 2.f * c / (d4.y + sqrtf(d4.y * d4.y + 4.f * lam * c)) : 0.f;
        c = w4.z * a4.z; o.z = d4.z > 0.f ? 2.f * c / (d4.z + sqrtf(d4.z * d4.z + 4.f * lam * c)) : 0.f;
        c = w4.w * a4.w; o.w = d4.w > 0.f ? 2.f * c / (d4.w + sqrtf(d4.w * d4.w + 4.f * lam * c)) : 0.f;
    } else {
        o.x = w4.x * a4.x / (d4.x + lam * w4.x + 1e-9f);
        o.y = w4.y * a4.y / (d4.y + lam * w4.y + 1e-9f);
        o.z = w4.z * a4.z / (d4.z + lam * w4.z + 1e-9f);
        o.w = w4.w * a4.w / (d4.w + lam * w4.w + 1e-9f);
    }
    const int c0 = lig * 4;
    if (c0 + 0 >= k) o.x = 0.f;
    if (c0 + 1 >= k) o.y = 0.f;
    if (c0 + 2 >= k) o.z = 0.f;
    if (c0 + 3 >= k) o.w = 0.f;
    return o;
}
template <bool KL, bool IS = false>
__device__ __forceinline__ void sp_epilogue_masked(float4 w4, float4 a4, float4 d4, float lam, int k, float* __restrict__ out_row,
                                                   int lig, int grp)
{
    const float4 o = sp_epilogue_masked_value<KL, IS>(w4, a4, d4, lam, k, lig);
    if (grp == 0) *reinterpret_cast<float4*>(out_row + lig * 4) = o;
}

// One phase over the units of one orientation.
//   Own [rows][KP]: the factor being updated (read), Out: where its update goes (may be Own: rows are owned by one wave),
//   Other [*][KP]: the factor gathered per non-zero, G (KP x KP f32) / S (KP f32): the other factor's Gram / sums.
//   OBJ: objective partial of the pair (Own, Other) per block into obj_part (Euclidean: Sum x wh; KL: Sum x log(x/wh) - x;
//   MASKED: Euclidean Sum (x - wh)^2, KL Sum x log(x/wh) - x + wh).
//   UPDATE: accumulate and run the epilogue (whole rows) or store the piece's sum (pieces).
//   MASKED: also accumulate the denominator (Sum wh h / Sum h) and run the masked epilogue; pieces store [sum | denominator].
template <int KP, bool KL, bool OBJ, bool UPDATE, bool MASKED, bool IS = false>
__global__ __launch_bounds__(64 * SP_WAVES) void sp_phase_kernel(
    const SpUnit* __restrict__ units, int64_t nunits, const int32_t* __restrict__ idx, const float* __restrict__ val,
    const float* __restrict__ Other, const float* Own, float* Out, const float* __restrict__ Gf, const float* __restrict__ S,
    float* __restrict__ slab, double* __restrict__ obj_part, float lam, int k, const int* flag)
{
    if (flag && *flag) return;
    constexpr int G = KP / 4, NG = 64 / G;
    constexpr bool GLDS = UPDATE && !KL && !MASKED && KP <= 128;
    __shared__ __attribute__((aligned(16))) float gs[GLDS ? KP * KP : 4];
    __shared__ double ob[SP_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lig = lane % G, grp = lane / G;
    if constexpr (GLDS) {
        for (int i = tid * 4; i < KP * KP; i += 64 * SP_WAVES * 4)
            *reinterpret_cast<float4*>(gs + i) = *reinterpret_cast<const float4*>(Gf + i);
        __syncthreads();
    }
    const float* Gsrc = GLDS ? gs : Gf;
    double objacc = 0.0;
    for (int64_t u = (int64_t)blockIdx.x * SP_WAVES + wave; u < nunits; u += (int64_t)gridDim.x * SP_WAVES) {
        const SpUnit U = units[u];
        const float4 w4 = *reinterpret_cast<const float4*>(Own + (int64_t)U.row * KP + lig * 4);
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        float4 den = make_float4(0.f, 0.f, 0.f, 0.f);     // (MASKED only)
        const long long end = U.beg + U.len;
        for (long long e0 = U.beg + grp; e0 < end; e0 += 4 * NG) {
            int c[4]; float x[4]; bool ok[4]; float4 h[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const long long e = e0 + (long long)t * NG;
                ok[t] = e < end;
                c[t] = ok[t] ? idx[e] : 0;
                x[t] = ok[t] ? val[e] : 0.f;
            }
#pragma unroll
            for (int t = 0; t < 4; ++t) h[t] = *reinterpret_cast<const float4*>(Other + (int64_t)c[t] * KP + lig * 4);
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                double wh = (double)w4.x * h[t].x + (double)w4.y * h[t].y + (double)w4.z * h[t].z + (double)w4.w * h[t].w;
#pragma unroll
                for (int off = 1; off < G; off <<= 1) wh += __shfl_xor(wh, off, 64);
                if constexpr (OBJ) {
                    if (lig == 0 && ok[t]) {
                        const double xv = x[t];
                        if constexpr (IS) {
                            const double r = xv / (wh + 1e-9);
                            objacc += r - log(r) - 1.0;
                        } else if constexpr (KL) {
                            double tl = xv * log(xv / wh);
                            if (tl == INFINITY || tl != tl) tl = 0.0;      // np.where(t == inf, 0, t); np.where(isnan(t), 0, t)
                            if constexpr (MASKED) objacc += tl - xv + wh;
                            else objacc += tl - xv;
                        } else if constexpr (MASKED) {
                            const double d = xv - wh;
                            objacc += d * d;
                        } else {
                            objacc += xv * wh;
                        }
                    }
                }
                if constexpr (UPDATE && IS) {          // (a slot past the unit's end: x = 0 and weight 0)
                    const double iq = 1.0 / (wh + 1e-9);
                    const float q = (float)((double)x[t] * iq * iq), r = ok[t] ? (float)iq : 0.f;
                    acc.x = fmaf(q, h[t].x, acc.x); acc.y = fmaf(q, h[t].y, acc.y);
                    acc.z = fmaf(q, h[t].z, acc.z); acc.w = fmaf(q, h[t].w, acc.w);
                    den.x = fmaf(r, h[t].x, den.x); den.y = fmaf(r, h[t].y, den.y);
                    den.z = fmaf(r, h[t].z, den.z); den.w = fmaf(r, h[t].w, den.w);
                } else if constexpr (UPDATE) {
                    const float q = KL ? (float)((double)x[t] / (wh + 1e-9)) : x[t];
                    acc.x = fmaf(q, h[t].x, acc.x); acc.y = fmaf(q, h[t].y, acc.y);
                    acc.z = fmaf(q, h[t].z, acc.z); acc.w = fmaf(q, h[t].w, acc.w);
                    if constexpr (MASKED) {            // (a slot past the unit's end gathered row 0: weight 0)
                        const float r = !ok[t] ? 0.f : KL ? 1.f : (float)wh;
                        den.x = fmaf(r, h[t].x, den.x); den.y = fmaf(r, h[t].y, den.y);
                        den.z = fmaf(r, h[t].z, den.z); den.w = fmaf(r, h[t].w, den.w);
                    }
                }
            }
        }
        if constexpr (UPDATE && MASKED) {
            acc = sp_sum_groups<G>(acc);
            den = sp_sum_groups<G>(den);
            if (U.slot >= 0) {
                if (grp == 0) {
                    float* p = slab + (int64_t)U.slot * (2 * KP) + lig * 4;
                    *reinterpret_cast<float4*>(p) = acc;
                    *reinterpret_cast<float4*>(p + KP) = den;
                }
            } else {
                sp_epilogue_masked<KL, IS>(w4, acc, den, lam, k, Out + (int64_t)U.row * KP, lig, grp);
            }
        } else if constexpr (UPDATE) {
            acc = sp_sum_groups<G>(acc);
            if (U.slot >= 0) {
                if (grp == 0) *reinterpret_cast<float4*>(slab + (int64_t)U.slot * KP + lig * 4) = acc;
            } else {
                sp_epilogue<KP, KL>(w4, acc, Gsrc, S, lam, k, Out + (int64_t)U.row * KP, lig, grp);
            }
        }
    }
    if constexpr (OBJ) {
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) objacc += __shfl_xor(objacc, off, 64);
        if (lane == 0) ob[wave] = objacc;
        __syncthreads();
        if (tid == 0) {
            double s = 0.0;
            for (int w = 0; w < SP_WAVES; ++w) s += ob[w];
            obj_part[blockIdx.x] = s;
        }
    }
}

// Rows split into pieces: the pieces' sums added in piece order (group g takes pieces g, g + NG, ..., then the groups'
// butterfly), then the epilogue.  MASKED: the same for both halves of a piece's [sum | denominator], then the masked epilogue.
template <int KP, bool KL, bool MASKED, bool IS = false>
__global__ __launch_bounds__(64 * SP_WAVES) void sp_fixup_kernel(
    const SpLong* __restrict__ longs, int64_t nlong, const float* __restrict__ slab, const float* Own, float* Out,
    const float* __restrict__ Gf, const float* __restrict__ S, float lam, int k, const int* flag)
{
    if (flag && *flag) return;
    constexpr int G = KP / 4, NG = 64 / G;
    if constexpr (MASKED) {
        const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lig = lane % G, grp = lane / G;
        for (int64_t l = (int64_t)blockIdx.x * SP_WAVES + wave; l < nlong; l += (int64_t)gridDim.x * SP_WAVES) {
            const SpLong L = longs[l];
            const float4 w4 = *reinterpret_cast<const float4*>(Own + (int64_t)L.row * KP + lig * 4);
            float4 acc = make_float4(0.f, 0.f, 0.f, 0.f), den = make_float4(0.f, 0.f, 0.f, 0.f);
            for (int p = grp; p < L.npieces; p += NG) {
                const float* s = slab + (int64_t)(L.slot0 + p) * (2 * KP) + lig * 4;
                acc = sp_add4(acc, *reinterpret_cast<const float4*>(s));
                den = sp_add4(den, *reinterpret_cast<const float4*>(s + KP));
            }
            acc = sp_sum_groups<G>(acc);
            den = sp_sum_groups<G>(den);
            sp_epilogue_masked<KL, IS>(w4, acc, den, lam, k, Out + (int64_t)L.row * KP, lig, grp);
        }
        return;
    }
    constexpr bool GLDS = !KL && !MASKED && KP <= 128;
    __shared__ __attribute__((aligned(16))) float gs[GLDS ? KP * KP : 4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lig = lane % G, grp = lane / G;
    if constexpr (GLDS) {
        for (int i = tid * 4; i < KP * KP; i += 64 * SP_WAVES * 4)
            *reinterpret_cast<float4*>(gs + i) = *reinterpret_cast<const float4*>(Gf + i);
        __syncthreads();
    }
    const float* Gsrc = GLDS ? gs : Gf;
    for (int64_t l = (int64_t)blockIdx.x * SP_WAVES + wave; l < nlong; l += (int64_t)gridDim.x * SP_WAVES) {
        const SpLong L = longs[l];
        const float4 w4 = *reinterpret_cast<const float4*>(Own + (int64_t)L.row * KP + lig * 4);
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int p = grp; p < L.npieces; p += NG)
            acc = sp_add4(acc, *reinterpret_cast<const float4*>(slab + (int64_t)(L.slot0 + p) * KP + lig * 4));
        acc = sp_sum_groups<G>(acc);
        sp_epilogue<KP, KL>(w4, acc, Gsrc, S, lam, k, Out + (int64_t)L.row * KP, lig, grp);
    }
}

// Per-slab f64 partials of F^T F (KP x KP) and of the column sums of F [R][KP]: block (slab, tile) covers rows
// [s * rps, (s + 1) * rps) and the TD x TD tile (ti, tj) of the Gram; tiles with tj = 0 also sum their columns.
template <int KP>
__global__ __launch_bounds__(256) void sp_stats_kernel(const float* __restrict__ F, int64_t R, int64_t rps,
                                                       double* __restrict__ part, const int* flag)
{
    if (flag && *flag) return;
    constexpr int TD = KP < 64 ? KP : 64, T = KP / TD, NO = TD * TD >= 256 ? TD * TD / 256 : 1;
    __shared__ float a[16][TD], b[16][TD];
    const int tid = threadIdx.x, s = blockIdx.x, ti = blockIdx.y / T, tj = blockIdx.y % T;
    const int64_t r0 = (int64_t)s * rps, r1 = std::min<int64_t>(R, r0 + rps);
    double acc[NO], cs = 0.0;
#pragma unroll
    for (int o = 0; o < NO; ++o) acc[o] = 0.0;
    for (int64_t rc = r0; rc < r1; rc += 16) {
        for (int i = tid; i < 16 * TD; i += 256) {
            const int rr = i / TD, cc = i % TD;
            const int64_t r = rc + rr;
            a[rr][cc] = r < r1 ? F[r * KP + ti * TD + cc] : 0.f;
            b[rr][cc] = r < r1 ? F[r * KP + tj * TD + cc] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int o = 0; o < NO; ++o) {
            const int e = tid + 256 * o;
            if (e < TD * TD) {
                const int p = e / TD, q = e % TD;
#pragma unroll
                for (int rr = 0; rr < 16; ++rr) acc[o] = fma((double)a[rr][p], (double)b[rr][q], acc[o]);
            }
        }
        if (tj == 0 && tid < TD)
            for (int rr = 0; rr < 16; ++rr) cs += (double)a[rr][tid];
        __syncthreads();
    }
    double* out = part + (int64_t)s * (KP * KP + KP);
#pragma unroll
    for (int o = 0; o < NO; ++o) {
        const int e = tid + 256 * o;
        if (e < TD * TD) out[(ti * TD + e / TD) * KP + tj * TD + e % TD] = acc[o];
    }
    if (tj == 0 && tid < TD) out[KP * KP + ti * TD + tid] = cs;
}

// Slabs summed in slab order: [0, kp^2) the Gram, [kp^2, kp^2 + kp) the column sums; f64 and f32 copies.
__global__ void sp_stats_reduce_kernel(const double* __restrict__ part, int slabs, int kp, double* __restrict__ g64, float* __restrict__ gf,
                                       double* __restrict__ c64, float* __restrict__ cf, const int* flag)
{
    if (flag && *flag) return;
    const int e = blockIdx.x * blockDim.x + threadIdx.x, kk = kp * kp;
    if (e >= kk + kp) return;
    double s = 0.0;
    for (int i = 0; i < slabs; ++i) s += part[(int64_t)i * (kk + kp) + e];
    if (e < kk) { g64[e] = s; gf[e] = (float)s; }
    else { c64[e - kk] = s; cf[e - kk] = (float)s; }
}

// The objective of the pair from the block partials (block order, then a fixed tree) and the small terms; recorded as
// obj[j] with the reference's stop rule (record) or only stored to *out.  MASKED: the block partials alone (KL: their sum,
// Euclidean: half of it).
template <bool KL, bool MASKED, bool IS = false>
__global__ __launch_bounds__(256) void sp_objective_kernel(
    const double* __restrict__ part, int nblk, const double* __restrict__ gw, const double* __restrict__ gh,
    const double* __restrict__ cw, const double* __restrict__ ch, int kp, double x2, double* __restrict__ out, int record,
    long long j, long long min_iter, double tol1, double tol2, DevState* __restrict__ st, double* __restrict__ obj_hist)
{
    if (record && st->flag) return;
    __shared__ double r[2][256];
    const int tid = threadIdx.x;
    double s = 0.0, t = 0.0;
    for (int i = tid; i < nblk; i += 256) s += part[i];
    if constexpr (!MASKED) {
        if (KL) { for (int c = tid; c < kp; c += 256) t += cw[c] * ch[c]; }
        else { for (int e = tid; e < kp * kp; e += 256) t += gw[e] * gh[e]; }
    }
    r[0][tid] = s; r[1][tid] = t;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) { r[0][tid] += r[0][tid + w]; r[1][tid] += r[1][tid + w]; }
        __syncthreads();
    }
    if (tid == 0) {
        const double obj = MASKED ? (KL || IS ? r[0][0] : 0.5 * r[0][0])
                                  : KL ? r[0][0] + r[1][0] : 0.5 * (x2 - 2.0 * r[0][0] + r[1][0]);
        *out = obj;
        if (record) nmfx_record_objective(st, obj_hist, obj, j, min_iter, tol1, tol2, true);
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------
template <typename T>
static int sp_alloc(nmfx_engine* E, T** p, int64_t count) {
    NMFX_HIP(hipMalloc(reinterpret_cast<void**>(p), (size_t)std::max<int64_t>(count, 1) * sizeof(T)));
    NMFX_HIP(hipMemsetAsync(*p, 0, (size_t)std::max<int64_t>(count, 1) * sizeof(T), E->stream));
    return NMFX_OK;
}

static int stat_slabs(int kp, int64_t R) {
    const int T = kp < 64 ? 1 : kp / 64;
    const int64_t smax = std::max(16, 256 / (T * T));
    return (int)std::min<int64_t>(smax, std::max<int64_t>(1, (R + 1023) / 1024));
}

int nmfx_sparse_init(nmfx_engine* E, int64_t nnz) {
    nmfx_sparse* S = new nmfx_sparse();
    E->sp = S;
    S->nnz = nnz;
    const int64_t kp = E->kp;
    int rc;
    if ((rc = sp_alloc(E, &E->W[0], E->m * kp))) return rc;
    if ((rc = sp_alloc(E, &E->W[1], E->m * kp))) return rc;
    if ((rc = sp_alloc(E, &S->Ht, E->n * kp))) return rc;
    for (int f = 0; f < 2; ++f) {
        if ((rc = sp_alloc(E, &S->g64[f], kp * kp))) return rc;
        if ((rc = sp_alloc(E, &S->gf[f], kp * kp))) return rc;
        if ((rc = sp_alloc(E, &S->cs64[f], kp))) return rc;
        if ((rc = sp_alloc(E, &S->csf[f], kp))) return rc;
        if ((rc = sp_alloc(E, &S->side[f].idx, nnz))) return rc;
        if ((rc = sp_alloc(E, &S->side[f].val, nnz))) return rc;
    }
    S->side[0].rows = E->m; S->side[1].rows = E->n;
    const int slabs = std::max(stat_slabs((int)kp, E->m), stat_slabs((int)kp, E->n));
    if ((rc = sp_alloc(E, &S->stat_part, (int64_t)slabs * (kp * kp + kp)))) return rc;
    S->obj_cap = 4 * E->ncu + 64;
    if ((rc = sp_alloc(E, &S->obj_part, S->obj_cap))) return rc;
    NMFX_HIP(hipStreamSynchronize(E->stream));
    return NMFX_OK;
}

void nmfx_sparse_free(nmfx_engine* E) {
    nmfx_sparse* S = E->sp;
    if (!S) return;
    void* bufs[] = {S->Ht, S->g64[0], S->g64[1], S->gf[0], S->gf[1], S->cs64[0], S->cs64[1], S->csf[0], S->csf[1],
                    S->stat_part, S->obj_part, S->hals_part, S->hals_r32, S->hals_r64, S->foldin_sweeps, S->mur_foldin_iters};
    for (void* b : bufs) if (b) hipFree(b);
    for (auto& sd : S->side) {
        void* sb[] = {sd.idx, sd.val, sd.units, sd.longs, sd.slab, sd.slab64};
        for (void* b : sb) if (b) hipFree(b);
    }
    delete S;
    E->sp = nullptr;
}

// Units of one orientation from its pointer array: whole rows, and rows longer than SP_CHUNK cut into pieces.
static int build_side(nmfx_engine* E, SpSide& sd, const int64_t* ptr) {
    std::vector<SpUnit> units;
    std::vector<SpLong> longs;
    units.reserve((size_t)sd.rows);
    int slot = 0;
    for (int64_t r = 0; r < sd.rows; ++r) {
        const int64_t b = ptr[r], len = ptr[r + 1] - ptr[r];
        if (len <= SP_CHUNK) { units.push_back({(long long)b, (int)r, (int)len, -1, 0}); continue; }
        const int np = (int)((len + SP_CHUNK - 1) / SP_CHUNK);
        longs.push_back({(int)r, slot, np, (int)units.size()});
        for (int p = 0; p < np; ++p)
            units.push_back({(long long)(b + (int64_t)p * SP_CHUNK), (int)r, (int)std::min<int64_t>(SP_CHUNK, len - (int64_t)p * SP_CHUNK), slot + p, 0});
        slot += np;
    }
    for (void* b : {(void*)sd.units, (void*)sd.longs, (void*)sd.slab, (void*)sd.slab64}) if (b) hipFree(b);
    sd.units = nullptr; sd.longs = nullptr; sd.slab = nullptr; sd.slab64 = nullptr;
    sd.npieces = slot;
    sd.nunits = (int64_t)units.size(); sd.nlong = (int64_t)longs.size();
    int rc;
    if ((rc = sp_alloc(E, &sd.units, sd.nunits))) return rc;
    if ((rc = sp_alloc(E, &sd.longs, sd.nlong))) return rc;
    if ((rc = sp_alloc(E, &sd.slab, (int64_t)slot * E->kp * (E->sp->masked ? 2 : 1)))) return rc;
    if (sd.nunits) NMFX_HIP(hipMemcpyAsync(sd.units, units.data(), units.size() * sizeof(SpUnit), hipMemcpyHostToDevice, E->stream));
    if (sd.nlong) NMFX_HIP(hipMemcpyAsync(sd.longs, longs.data(), longs.size() * sizeof(SpLong), hipMemcpyHostToDevice, E->stream));
    NMFX_HIP(hipStreamSynchronize(E->stream));
    sd.nblk = (int)std::max<int64_t>(1, std::min<int64_t>(4 * E->ncu, (sd.nunits + SP_WAVES - 1) / SP_WAVES));
    return NMFX_OK;
}

extern "C" int nmfx_upload_csr(nmfx_handle_t E, const int64_t* row_ptr, const int32_t* col_idx, const void* values, int dtype) {
    if (!E) return NMFX_E_ARG;
    if (!E->sp) { E->err = "upload_csr: not a sparse handle (nmfx_create_csr)"; return NMFX_E_ARG; }
    nmfx_sparse* S = E->sp;
    const int64_t m = E->m, n = E->n, nnz = S->nnz;
    if (!row_ptr || (nnz > 0 && (!col_idx || !values))) { E->err = "upload_csr: NULL array"; return NMFX_E_ARG; }
    if (dtype != NMFX_F32 && dtype != NMFX_F64) { E->err = "upload_csr: dtype must be NMFX_F32 or NMFX_F64"; return NMFX_E_ARG; }
    if (row_ptr[0] != 0 || row_ptr[m] != nnz) { E->err = "upload_csr: row_ptr[0] must be 0 and row_ptr[m] the nnz of nmfx_create_csr"; return NMFX_E_ARG; }
    for (int64_t r = 0; r < m; ++r)          // (the whole row_ptr before any col_idx / values entry is read)
        if (row_ptr[r + 1] < row_ptr[r] || row_ptr[r + 1] > nnz) { E->err = "upload_csr: row_ptr must not decrease nor exceed nnz"; return NMFX_E_ARG; }
    std::vector<float> v((size_t)nnz);
    double x2 = 0.0;
    for (int64_t r = 0; r < m; ++r) {
        for (int64_t e = row_ptr[r]; e < row_ptr[r + 1]; ++e) {
            const int32_t c = col_idx[e];
            if (c < 0 || c >= n || (e > row_ptr[r] && c <= col_idx[e - 1])) {
                E->err = "upload_csr: column indices must lie in [0, n) and increase strictly within a row (no duplicates)"; return NMFX_E_ARG; }
            const float x = dtype == NMFX_F32 ? static_cast<const float*>(values)[e] : (float)static_cast<const double*>(values)[e];
            if (!(x >= 0.f)) { E->err = "upload_csr: values must be non-negative (MUR)"; return NMFX_E_ARG; }
            v[(size_t)e] = x;
            x2 += (double)x * (double)x;
        }
    }
    // CSC by a counting sort over the rows in order: rows ascend within every column (deterministic)
    std::vector<int64_t> cptr((size_t)n + 1, 0);
    for (int64_t e = 0; e < nnz; ++e) cptr[(size_t)col_idx[e] + 1]++;
    for (int64_t c = 0; c < n; ++c) cptr[(size_t)c + 1] += cptr[(size_t)c];
    std::vector<int64_t> fill(cptr.begin(), cptr.end() - 1);
    std::vector<int32_t> ridx((size_t)nnz);
    std::vector<float> vt((size_t)nnz);
    for (int64_t r = 0; r < m; ++r)
        for (int64_t e = row_ptr[r]; e < row_ptr[r + 1]; ++e) {
            const int64_t d = fill[(size_t)col_idx[e]]++;
            ridx[(size_t)d] = (int32_t)r; vt[(size_t)d] = v[(size_t)e];
        }
    NMFX_HIP(hipSetDevice(E->device));
    if (nnz) {
        NMFX_HIP(hipMemcpyAsync(S->side[0].idx, col_idx, (size_t)nnz * 4, hipMemcpyHostToDevice, E->stream));
        NMFX_HIP(hipMemcpyAsync(S->side[0].val, v.data(), (size_t)nnz * 4, hipMemcpyHostToDevice, E->stream));
        NMFX_HIP(hipMemcpyAsync(S->side[1].idx, ridx.data(), (size_t)nnz * 4, hipMemcpyHostToDevice, E->stream));
        NMFX_HIP(hipMemcpyAsync(S->side[1].val, vt.data(), (size_t)nnz * 4, hipMemcpyHostToDevice, E->stream));
    }
    NMFX_HIP(hipStreamSynchronize(E->stream));
    int rc;
    if ((rc = build_side(E, S->side[0], row_ptr))) return rc;
    if ((rc = build_side(E, S->side[1], cptr.data()))) return rc;
    S->x2 = x2;
    E->have_v = true;
    return NMFX_OK;
}

// Between nmfx_create_csr and nmfx_upload_csr only: the stored entries become the observed set (the header's sparse block).
extern "C" int nmfx_set_masked(nmfx_handle_t E, int on) {
    if (!E) return NMFX_E_ARG;
    if (!E->sp) { E->err = "set_masked: not a sparse handle (nmfx_create_csr)"; return NMFX_E_ARG; }
    if (E->have_v) { E->err = "set_masked: call it before nmfx_upload_csr"; return NMFX_E_STATE; }
    E->sp->masked = on != 0;
    return NMFX_OK;
}

// ---- launchers --------------------------------------------------------------------------------------------------------
template <int KP>
static int launch_stats(nmfx_engine* E, const float* F, int64_t R, int f, const int* flag) {
    nmfx_sparse* S = E->sp;
    const int slabs = stat_slabs(KP, R), T = KP < 64 ? 1 : KP / 64;
    const int64_t rps = (R + slabs - 1) / slabs;
    hipLaunchKernelGGL((sp_stats_kernel<KP>), dim3(slabs, T * T), dim3(256), 0, E->stream, F, R, rps, S->stat_part, flag);
    const int tot = KP * KP + KP;
    hipLaunchKernelGGL(sp_stats_reduce_kernel, dim3((tot + 255) / 256), dim3(256), 0, E->stream, (const double*)S->stat_part, slabs, KP,
                       S->g64[f], S->gf[f], S->cs64[f], S->csf[f], flag);
    NMFX_HIP(hipGetLastError());
    return NMFX_OK;
}

// side 0: own W (Wold -> Wnew), gather H^T, other factor's stats 1; side 1: own H^T (in place), gather W, stats 0
// LOSS: NMFX_EU / NMFX_KL / NMFX_IS (the last on masked handles only: sp_ready)
template <int KP, int LOSS>
static int launch_phase(nmfx_engine* E, int side, const float* Own, float* Out, const float* Other, bool obj, bool update,
                        float lam, const int* flag) {
    constexpr bool KL = LOSS == NMFX_KL, IS = LOSS == NMFX_IS;
    nmfx_sparse* S = E->sp;
    SpSide& sd = S->side[side];
    const int o = 1 - side;
    const dim3 grid(sd.nblk), blk(64 * SP_WAVES);
#define SP_ARGS sd.units, sd.nunits, (const int32_t*)sd.idx, (const float*)sd.val, Other, Own, Out, (const float*)S->gf[o], \
                (const float*)S->csf[o], sd.slab, S->obj_part, lam, E->k, flag
    if constexpr (IS) {
        if (obj && update) hipLaunchKernelGGL((sp_phase_kernel<KP, false, true, true, true, true>), grid, blk, 0, E->stream, SP_ARGS);
        else if (obj) hipLaunchKernelGGL((sp_phase_kernel<KP, false, true, false, true, true>), grid, blk, 0, E->stream, SP_ARGS);
        else hipLaunchKernelGGL((sp_phase_kernel<KP, false, false, true, true, true>), grid, blk, 0, E->stream, SP_ARGS);
    } else if (S->masked) {
        if (obj && update) hipLaunchKernelGGL((sp_phase_kernel<KP, KL, true, true, true>), grid, blk, 0, E->stream, SP_ARGS);
        else if (obj) hipLaunchKernelGGL((sp_phase_kernel<KP, KL, true, false, true>), grid, blk, 0, E->stream, SP_ARGS);
        else hipLaunchKernelGGL((sp_phase_kernel<KP, KL, false, true, true>), grid, blk, 0, E->stream, SP_ARGS);
    } else {
        if (obj && update) hipLaunchKernelGGL((sp_phase_kernel<KP, KL, true, true, false>), grid, blk, 0, E->stream, SP_ARGS);
        else if (obj) hipLaunchKernelGGL((sp_phase_kernel<KP, KL, true, false, false>), grid, blk, 0, E->stream, SP_ARGS);
        else hipLaunchKernelGGL((sp_phase_kernel<KP, KL, false, true, false>), grid, blk, 0, E->stream, SP_ARGS);
    }
#undef SP_ARGS
    NMFX_HIP(hipGetLastError());
    if (update && sd.nlong) {
        const int nb = (int)std::min<int64_t>(4 * E->ncu, (sd.nlong + SP_WAVES - 1) / SP_WAVES);
        auto fix = IS ? sp_fixup_kernel<KP, false, true, IS> : S->masked ? sp_fixup_kernel<KP, KL, true> : sp_fixup_kernel<KP, KL, false>;
        hipLaunchKernelGGL(fix, dim3(nb), blk, 0, E->stream, (const SpLong*)sd.longs, sd.nlong,
                           (const float*)sd.slab, Own, Out, (const float*)S->gf[o], (const float*)S->csf[o], lam, E->k, flag);
        NMFX_HIP(hipGetLastError());
    }
    return NMFX_OK;
}

static int launch_objective(nmfx_engine* E, int loss, double* out, bool record, int64_t j, int64_t min_iter, double tol1, double tol2) {
    nmfx_sparse* S = E->sp;
    const bool kl = loss == NMFX_KL;
    auto kern = loss == NMFX_IS ? sp_objective_kernel<false, true, true> : S->masked ? (kl ? sp_objective_kernel<true, true> : sp_objective_kernel<false, true>)
                          : (kl ? sp_objective_kernel<true, false> : sp_objective_kernel<false, false>);
    hipLaunchKernelGGL(kern, dim3(1), dim3(256), 0, E->stream, (const double*)S->obj_part, S->side[0].nblk,
                       (const double*)S->g64[0], (const double*)S->g64[1], (const double*)S->cs64[0], (const double*)S->cs64[1],
                       E->kp, S->x2, out, record ? 1 : 0, (long long)j, (long long)min_iter, tol1, tol2, E->state, E->obj_hist);
    NMFX_HIP(hipGetLastError());
    return NMFX_OK;
}

// one phase launch for a run-time loss
template <int KP>
static int phase_for(nmfx_engine* E, int loss, int side, const float* Own, float* Out, const float* Other, bool obj, bool update,
                     float lam, const int* flag) {
    switch (loss) {
        case NMFX_IS: return launch_phase<KP, NMFX_IS>(E, side, Own, Out, Other, obj, update, lam, flag);
        case NMFX_KL: return launch_phase<KP, NMFX_KL>(E, side, Own, Out, Other, obj, update, lam, flag);
        default: return launch_phase<KP, NMFX_EU>(E, side, Own, Out, Other, obj, update, lam, flag);
    }
}

template <int KP>
static int sp_iteration(nmfx_engine* E, int loss, double lw, double lh, int64_t min_iter, double tol1, double tol2, int64_t j) {
    nmfx_sparse* S = E->sp;
    const int* flag = &E->state->flag;
    const float* Wold = E->W[j & 1];
    float* Wnew = E->W[(j + 1) & 1];
    int rc;
    { ProfScope ps(E, "sp_wphase");
      rc = phase_for<KP>(E, loss, 0, Wold, Wnew, S->Ht, true, true, (float)lw, flag);
      if (rc) return rc; }
    if ((rc = launch_objective(E, loss, E->xf64, true, j, min_iter, tol1, tol2))) return rc;
    if (!S->masked) {                 // (a masked update takes its denominators from the phase itself)
      ProfScope ps(E, "sp_stats");
      if ((rc = launch_stats<KP>(E, Wnew, E->m, 0, flag))) return rc; }
    { ProfScope ps(E, "sp_hphase");
      rc = phase_for<KP>(E, loss, 1, S->Ht, S->Ht, Wnew, false, true, (float)lh, flag);
      if (rc) return rc; }
    if (!S->masked) {
      ProfScope ps(E, "sp_stats");
      if ((rc = launch_stats<KP>(E, S->Ht, E->n, 1, flag))) return rc; }
    E->run.wsel = (int)((j + 1) & 1);
    return NMFX_OK;
}

// objective pass of (W[wsel or j & 1], H) without an update
template <int KP>
static int sp_objective_pass(nmfx_engine* E, int loss, const float* W, const int* flag) {
    return phase_for<KP>(E, loss, 0, W, nullptr, E->sp->Ht, true, false, 0.f, flag);
}

#define SP_DISPATCH(call) \
    switch (E->kp) { case 4: rc = call<4>; break; case 8: rc = call<8>; break; case 16: rc = call<16>; break; \
                     case 32: rc = call<32>; break; case 64: rc = call<64>; break; case 128: rc = call<128>; break; \
                     default: rc = call<256>; break; }

static int sp_ready(nmfx_engine* E, int distance, int64_t first, int64_t count) {
    nmfx_entry a = {NMFX_FAM_MUR, first, count, NMFX_D_NONE, NMFX_D_NONE};      // (a sparse handle derives nothing from (W, H) that outlives a call)
    if (distance == NMFX_IS && !E->sp->masked)
        a.bad = "the Itakura-Saito divergence (IS) is infinite at the zeros of an unmasked sparse V: make the handle masked (nmfx_set_masked)";
    else if (distance != NMFX_EU && distance != NMFX_KL && distance != NMFX_IS) a.bad = "Unknown distance type.";
    else if (first < 0 || count < 0) a.bad = "negative iteration range";
    int rc = nmfx_enter(E, a); if (rc) return rc;
    E->run.mur_loss(distance);
    return NMFX_OK;
}

int nmfx_sparse_mur_run(nmfx_engine* E, int distance, double lw, double lh, int64_t min_iter, double tol1, double tol2,
                        int64_t first, int64_t count) {
    int rc = sp_ready(E, distance, first, count); if (rc) return rc;
    if (E->sp->mur_foldin_done) { E->sp->mur_foldin_done = false; E->run.w_in_place = false; }      // (W ping-pongs again: a fold-in needs new factors)
    for (int64_t j = first; j < first + count && !rc; ++j) {
#define SP_IT(KP) sp_iteration<KP>(E, distance, lw, lh, min_iter, tol1, tol2, j)
        switch (E->kp) { case 4: rc = SP_IT(4); break; case 8: rc = SP_IT(8); break; case 16: rc = SP_IT(16); break;
                         case 32: rc = SP_IT(32); break; case 64: rc = SP_IT(64); break; case 128: rc = SP_IT(128); break;
                         default: rc = SP_IT(256); break; }
#undef SP_IT
    }
    return rc;
}

static int objective_pass(nmfx_engine* E, int loss, const float* W, const int* flag) {
    int rc;
#define SP_OP(KP) sp_objective_pass<KP>(E, loss, W, flag)
    switch (E->kp) { case 4: rc = SP_OP(4); break; case 8: rc = SP_OP(8); break; case 16: rc = SP_OP(16); break;
                     case 32: rc = SP_OP(32); break; case 64: rc = SP_OP(64); break; case 128: rc = SP_OP(128); break;
                     default: rc = SP_OP(256); break; }
#undef SP_OP
    return rc;
}

int nmfx_sparse_mur_finish(nmfx_engine* E, int distance, int64_t min_iter, double tol1, double tol2, int64_t done) {
    int rc = sp_ready(E, distance, done, 0); if (rc) return rc;
    if ((rc = objective_pass(E, distance, E->W[done & 1], &E->state->flag))) return rc;
    return launch_objective(E, distance, E->xf64, true, done, min_iter, tol1, tol2);
}

// After the stop rule has fired, the launches behind it in the batch did nothing: the current W of a MUR run is the one of
// the pair at the stop (W[(stop_i + 1) & 1]), whose Gram is still in g64[0].
static int sync_wsel(nmfx_engine* E) {
    NMFX_HIP(hipSetDevice(E->device));
    DevState hs;
    NMFX_HIP(hipMemcpyAsync(&hs, E->state, sizeof(DevState), hipMemcpyDeviceToHost, E->stream));
    NMFX_HIP(hipStreamSynchronize(E->stream));
    if (hs.flag && !E->run.w_in_place) E->run.wsel = (int)((hs.stop_i + 1) & 1);      // (sparse HALS updates W[0] in place)
    return NMFX_OK;
}

int nmfx_sparse_objective_f64(nmfx_engine* E, double* out) {
    if (!E->have_v || !E->have_f) { E->err = "upload the CSR matrix and set factors first"; return NMFX_E_STATE; }
    int rc;
    if ((rc = sync_wsel(E))) return rc;
    if ((rc = objective_pass(E, NMFX_EU, E->W[E->run.wsel], nullptr))) return rc;
    if ((rc = launch_objective(E, NMFX_EU, E->xf64 + 1, false, 0, 0, 0.0, 0.0))) return rc;
    NMFX_HIP(hipMemcpyAsync(out, E->xf64 + 1, sizeof(double), hipMemcpyDeviceToHost, E->stream));
    NMFX_HIP(hipStreamSynchronize(E->stream));
    return NMFX_OK;
}

static int stats_both(nmfx_engine* E) {
    int rc = NMFX_OK;
#define SP_ST(KP) (launch_stats<KP>(E, E->W[0], E->m, 0, nullptr) ? NMFX_E_HIP : launch_stats<KP>(E, E->sp->Ht, E->n, 1, nullptr))
    switch (E->kp) { case 4: rc = SP_ST(4); break; case 8: rc = SP_ST(8); break; case 16: rc = SP_ST(16); break;
                     case 32: rc = SP_ST(32); break; case 64: rc = SP_ST(64); break; case 128: rc = SP_ST(128); break;
                     default: rc = SP_ST(256); break; }
#undef SP_ST
    return rc;
}

int nmfx_sparse_set_factors(nmfx_engine* E, const double* w, const double* hmat) {
    NMFX_HIP(hipSetDevice(E->device));
    const int64_t m = E->m, n = E->n, k = E->k, kp = E->kp;
    if (w) {
        std::vector<float> t((size_t)(m * kp), 0.f);
        for (int64_t r = 0; r < m; ++r)
            for (int64_t c = 0; c < k; ++c) t[(size_t)(r * kp + c)] = (float)w[r * k + c];
        NMFX_HIP(hipMemcpyAsync(E->W[0], t.data(), t.size() * 4, hipMemcpyHostToDevice, E->stream));
        NMFX_HIP(hipMemsetAsync(E->W[1], 0, t.size() * 4, E->stream));
        NMFX_HIP(hipStreamSynchronize(E->stream));
    }
    if (hmat) {
        std::vector<float> t((size_t)(n * kp), 0.f);
        for (int64_t c = 0; c < k; ++c)
            for (int64_t j = 0; j < n; ++j) t[(size_t)(j * kp + c)] = (float)hmat[c * n + j];
        NMFX_HIP(hipMemcpyAsync(E->sp->Ht, t.data(), t.size() * 4, hipMemcpyHostToDevice, E->stream));
        NMFX_HIP(hipStreamSynchronize(E->stream));
    }
    E->have_f = true;
    E->derived.void_all_but(NMFX_D_NONE);
    E->run.reset();
    E->sp->foldin_done = false;
    E->sp->mur_foldin_done = false;
    int rc;
    if (!E->sp->masked && (rc = stats_both(E))) return rc;
    NMFX_HIP(hipStreamSynchronize(E->stream));
    return NMFX_OK;
}

int nmfx_sparse_get_factors(nmfx_engine* E, double* w, double* hmat) {
    int rc;
    if ((rc = sync_wsel(E))) return rc;
    const int64_t m = E->m, n = E->n, k = E->k, kp = E->kp;
    if (w) {
        std::vector<float> t((size_t)(m * kp));
        NMFX_HIP(hipMemcpyAsync(t.data(), E->W[E->run.wsel], t.size() * 4, hipMemcpyDeviceToHost, E->stream));
        NMFX_HIP(hipStreamSynchronize(E->stream));
        for (int64_t r = 0; r < m; ++r)
            for (int64_t c = 0; c < k; ++c) w[r * k + c] = (double)t[(size_t)(r * kp + c)];
    }
    if (hmat) {
        std::vector<float> t((size_t)(n * kp));
        NMFX_HIP(hipMemcpyAsync(t.data(), E->sp->Ht, t.size() * 4, hipMemcpyDeviceToHost, E->stream));
        NMFX_HIP(hipStreamSynchronize(E->stream));
        for (int64_t c = 0; c < k; ++c)
            for (int64_t j = 0; j < n; ++j) hmat[c * n + j] = (double)t[(size_t)(j * kp + c)];
    }
    return NMFX_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// HALS on sparse V (nmfx_hals_sparse_run)
// ---------------------------------------------------------------------------------------------------------------------
// A half-step is, per owned row x of the factor being updated (a row of W, or a row of H^T = a column of H),
//     r = Sum_nz v * gathered row of the other factor,    G = the other factor's Gram + 2 lambda I,
// and `sweeps` projected Gauss-Seidel sweeps of kernels_hals.hip on (G, r) from x.  The wave that gathered r runs the sweep:
// after sp_sum_groups every group of G = KP / 4 lanes holds r and x as float4 per lane (variable j: lane j / 4 of its group,
// component j % 4), and the sweep stays in that layout -- all groups run it redundantly on the same bits.  The residual
// g = r - G x is formed once, row l of the LDS copy of G (= column l) against x_l broadcast from its lane; step j takes
//     delta = max(-x_j, g_j / G_jj) from variable j's lane (v_readlane),  x_j += delta,  g -= delta G[j][:]
// (the lane keeps -x_j, the lower bound of its step).  No wh, no butterfly per non-zero.  Loop bounds are wave-uniform
// (ceil(k / 4) lanes, sweeps, the unit index); padded components are written as exact zeros; a component with G_jj = 0
// keeps its value.  A piece of a long row stores its partial r in the slab; sp_hals_fixup_kernel adds the pieces in piece
// order and runs the same sweep.  The mat-vec and the step of this layout are written once, in sp_hals_sweeps<KP, SOLVE>:
// sp_hals_row calls it for the sparse kernels here, for masked HALS and, with SOLVE, for the fold-in of either.  The dense
// layout (one variable per lane and slot) has its own single copy in kernels_hals.hip; the two are not merged.
//
// CROSS (the H phase): r_c = W_new^T x_c is summed in f64 (products of f32 values are exact there) and rounded to f32 for
// the sweep only; after the sweep the wave adds <h_new_c, r_c> in f64 to its block's partial.  Summed over the columns that
// is Sum_nz x wh of the new pair, the one term of the Euclidean objective that needs the non-zeros: no third pass over them.
template <int KP>
__device__ __forceinline__ void sp_hals_stage(float* gs, const float* __restrict__ Gf, float diag_add, int k) {
    for (int i = threadIdx.x * 4; i < KP * KP; i += 64 * SP_WAVES * 4) {
        float4 v = *reinterpret_cast<const float4*>(Gf + i);
        const int row = i / KP, col = i % KP;
        if (row < k) {
            v.x += (col == row) ? diag_add : 0.f; v.y += (col + 1 == row) ? diag_add : 0.f;
            v.z += (col + 2 == row) ? diag_add : 0.f; v.w += (col + 3 == row) ? diag_add : 0.f;
        }
        *reinterpret_cast<float4*>(gs + i) = v;
    }
    __syncthreads();
}

// The sweeps of one owned row, written once for this layout.  x: the row (this lane's four components), g: in r, out the kept
// residual; on return x is the new row (padding 0, dead components as they were).  Returns the number of sweeps run.
// SOLVE (HALS fold-in): `sweeps` is the cap, and the row stops after the first sweep that moves no component by more
// than tol times the largest component.  d comes from v_readlane and is wave-uniform: the sweep keeps a running max |d|; the largest
// component is one butterfly over the group's lanes (every group holds the same bits; a dead component keeps its value and counts,
// padding does not); the test and the exit are wave-uniform.  The kept residual is formed anew from r (reload: g <- r) before the
// sweeps 17, 33, ...: the most a half-step ever carries it.  Without SOLVE none of that is compiled, so a count <= 16 leaves the
// bits of the plain sweep with that count.
template <int KP, bool SOLVE, typename RL>
__device__ __forceinline__ int sp_hals_sweeps(const float* gs, const float (&inv)[4], const bool (&live)[4], float (&x)[4],
                                              float (&g)[4], int k, int sweeps, float tol, int lig, RL reload)
{
    constexpr int G = KP / 4;
    const int nl = (k + 3) >> 2;                        // lanes of a group that hold a variable
    const float* grow = gs + lig * 4;
    float nx[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) nx[t] = live[t] ? -x[t] : 0.f;      // 0 with inv = 0 where G_jj = 0 or beyond k: a step of 0
    auto residual = [&]() {                             // g -= G x: the rows of a lane's four variables at a time
        for (int l4 = 0; l4 < nl; ++l4) {
            float4 c[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) c[t] = *reinterpret_cast<const float4*>(grow + (4 * l4 + t) * KP);
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const float xl = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x[t]), l4));
                g[0] = fmaf(-c[t].x, xl, g[0]); g[1] = fmaf(-c[t].y, xl, g[1]);
                g[2] = fmaf(-c[t].z, xl, g[2]); g[3] = fmaf(-c[t].w, xl, g[3]);
            }
        }
    };
    residual();
    int s = 0;
    while (SOLVE || s < sweeps) {                       // (SOLVE: left by the break below, at s = sweeps at the latest)
        [[maybe_unused]] float dmax = 0.f;
        for (int l4 = 0; l4 < nl; ++l4) {
            float4 c[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) c[t] = *reinterpret_cast<const float4*>(grow + (4 * l4 + t) * KP);
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const float cand = fmaxf(nx[t], g[t] * inv[t]);
                const float d = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(cand), l4));
                if constexpr (SOLVE) dmax = fmaxf(dmax, fabsf(d));
                nx[t] = (lig == l4) ? nx[t] - d : nx[t];           // (d = -x_j: an exact zero)
                g[0] = fmaf(-c[t].x, d, g[0]); g[1] = fmaf(-c[t].y, d, g[1]);
                g[2] = fmaf(-c[t].z, d, g[2]); g[3] = fmaf(-c[t].w, d, g[3]);
            }
        }
        ++s;
        if constexpr (SOLVE) {
            float xmax = 0.f;
#pragma unroll
            for (int t = 0; t < 4; ++t) xmax = fmaxf(xmax, live[t] ? 0.f - nx[t] : lig * 4 + t < k ? x[t] : 0.f);
#pragma unroll
            for (int off = 1; off < G; off <<= 1) xmax = fmaxf(xmax, __shfl_xor(xmax, off, 64));
            xmax = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(xmax)));
            if (dmax <= tol * xmax || s >= sweeps) break;
            if ((s & 15) == 0) {
#pragma unroll
                for (int t = 0; t < 4; ++t) x[t] = live[t] ? 0.f - nx[t] : x[t];
                reload(g);
                residual();
            }
        }
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) x[t] = lig * 4 + t >= k ? 0.f : live[t] ? 0.f - nx[t] : x[t];      // (0 - 0: +0)
    return s;
}

// this lane's reciprocals of the diagonal of the staged G
template <int KP>
__device__ __forceinline__ void sp_hals_diag(const float* gs, int k, int lig, float (&inv)[4], bool (&live)[4]) {
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int j = lig * 4 + t;
        const float gd = gs[j * KP + j];
        live[t] = j < k && gd > 0.f;
        inv[t] = live[t] ? 1.f / gd : 0.f;
    }
}

// One owned row with its summed right-hand side r (R = double on the CROSS side): the sweep, the row written by group 0, and
// on the CROSS side the row's <x_new, r> in f64 (returned on every lane of group 0; added by lane 0).
// SOLVE (fold-in): the stop rule of sp_hals_sweeps<SOLVE>, with `sweeps` its cap; lane 0 writes the row's sweep count to *count.
// rlds: where the row's r stays in LDS for the solve's refresh (masked HALS), or nullptr: r stays in this lane's registers.
template <int KP, bool CROSS, typename R, bool SOLVE = false>
__device__ __forceinline__ double sp_hals_row(const float* gs, const float (&inv)[4], const bool (&live)[4], const R (&r)[4],
                                              float* row, int k, int sweeps, int lig, int grp, float tol = 0.f,
                                              int32_t* count = nullptr, const float* rlds = nullptr)
{
    constexpr int G = KP / 4;
    const float4 x4 = *reinterpret_cast<const float4*>(row + lig * 4);
    float x[4] = {x4.x, x4.y, x4.z, x4.w};
    float g[4] = {(float)r[0], (float)r[1], (float)r[2], (float)r[3]};
    [[maybe_unused]] const int s = sp_hals_sweeps<KP, SOLVE>(gs, inv, live, x, g, k, sweeps, tol, lig, [&](float (&gg)[4]) {
        if (rlds) {
            const float4 r4 = *reinterpret_cast<const float4*>(rlds + lig * 4);
            gg[0] = r4.x; gg[1] = r4.y; gg[2] = r4.z; gg[3] = r4.w;
        } else {
#pragma unroll
            for (int t = 0; t < 4; ++t) gg[t] = (float)r[t];
        }
    });
    if constexpr (SOLVE) { if (grp == 0 && lig == 0) *count = s; }
    if (grp == 0) *reinterpret_cast<float4*>(row + lig * 4) = make_float4(x[0], x[1], x[2], x[3]);
    double cross = 0.0;
    if constexpr (CROSS) {
        cross = fma((double)x[0], (double)r[0], fma((double)x[1], (double)r[1], fma((double)x[2], (double)r[2], (double)x[3] * (double)r[3])));
#pragma unroll
        for (int off = 1; off < G; off <<= 1) cross += __shfl_xor(cross, off, 64);
    }
    return cross;
}

// the waves' objective sums -> the block's partial (every thread of the block calls)
__device__ __forceinline__ void sp_hals_block_partial(double objacc, double* ob, double* __restrict__ out) {
    const int tid = threadIdx.x;
    if ((tid & 63) == 0) ob[tid >> 6] = objacc;
    __syncthreads();
    if (tid == 0) {
        double s = 0.0;
        for (int w = 0; w < SP_WAVES; ++w) s += ob[w];
        *out = s;
    }
}

// r of one unit, the non-zeros [beg, beg + len): acc += Sum_e v_e Other[idx_e, :], this lane's four components, in f64 where
// CROSS.  Group grp of the wave takes the non-zeros grp, grp + NG, ..., four steps' gathers in flight; then the groups' sums are
// added by a fixed butterfly, so every lane ends with the same bits.  (At KP = 256 a group is the whole wave: NG = 1, four
// consecutive non-zeros in flight, no butterfly.)
template <int KP, bool CROSS, typename R>
__device__ __forceinline__ void sp_hals_gather(long long beg, int len, const int32_t* __restrict__ idx, const float* __restrict__ val,
                                               const float* __restrict__ Other, int lig, int grp, R (&acc)[4])
{
    constexpr int G = KP / 4, NG = 64 / G;
    const long long end = beg + len;
    for (long long e0 = beg + grp; e0 < end; e0 += 4 * NG) {
        int c[4]; float x[4]; float4 h[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const long long e = e0 + (long long)t * NG;
            const bool ok = e < end;
            c[t] = ok ? idx[e] : 0;
            x[t] = ok ? val[e] : 0.f;               // (a slot past the unit's end gathers row 0 with weight 0)
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) h[t] = *reinterpret_cast<const float4*>(Other + (int64_t)c[t] * KP + lig * 4);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            if constexpr (CROSS) {
                const double xv = x[t];
                acc[0] = fma(xv, (double)h[t].x, acc[0]); acc[1] = fma(xv, (double)h[t].y, acc[1]);
                acc[2] = fma(xv, (double)h[t].z, acc[2]); acc[3] = fma(xv, (double)h[t].w, acc[3]);
            } else {
                acc[0] = fmaf(x[t], h[t].x, acc[0]); acc[1] = fmaf(x[t], h[t].y, acc[1]);
                acc[2] = fmaf(x[t], h[t].z, acc[2]); acc[3] = fmaf(x[t], h[t].w, acc[3]);
            }
        }
    }
#pragma unroll
    for (int off = G; off < 64; off <<= 1) {        // the groups' sums: every lane ends with the same bits
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[t] += __shfl_xor(acc[t], off, 64);
    }
}

//   Own [rows][KP]: the factor being updated, in place (a row is owned by one wave; the gathers read the other factor only);
//   Other [*][KP]: the factor gathered per non-zero; Gf: its Gram (KP x KP f32), diag_add = (float)(2 lambda);
//   slab: the pieces' partial r, f32 (W phase) or f64 (CROSS); obj_part[blockIdx.x]: the block's Sum <x_new, r> (CROSS).
//   SOLVE (fold-in): every row is swept to the stop rule of sp_hals_sweeps<SOLVE> (tol; `sweeps` is the cap) and leaves its count in
//   counts[row].  The waves' trip counts then differ by more than the gather length: the only block barriers are the staging
//   one before the unit loop and the partial reduction behind it.
template <int KP, bool CROSS, bool SOLVE = false>
__global__ __launch_bounds__(64 * SP_WAVES) void sp_hals_phase_kernel(
    const SpUnit* __restrict__ units, int64_t nunits, const int32_t* __restrict__ idx, const float* __restrict__ val,
    const float* __restrict__ Other, float* Own, const float* __restrict__ Gf, float diag_add, void* __restrict__ slab,
    double* __restrict__ obj_part, int k, int sweeps, const int* flag, float tol = 0.f, int32_t* __restrict__ counts = nullptr)
{
    if (*flag) return;
    constexpr int G = KP / 4;
    using R = typename std::conditional<CROSS, double, float>::type;
    __shared__ __attribute__((aligned(16))) float gs[KP * KP];
    __shared__ double ob[SP_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lig = lane % G, grp = lane / G;
    sp_hals_stage<KP>(gs, Gf, diag_add, k);
    float inv[4]; bool live[4];
    sp_hals_diag<KP>(gs, k, lig, inv, live);
    double objacc = 0.0;
    for (int64_t u = (int64_t)blockIdx.x * SP_WAVES + wave; u < nunits; u += (int64_t)gridDim.x * SP_WAVES) {
        const SpUnit U = units[u];
        R acc[4] = {0, 0, 0, 0};
        sp_hals_gather<KP, CROSS>(U.beg, U.len, idx, val, Other, lig, grp, acc);
        if (U.slot >= 0) {                              // (wave-uniform)
            if (grp == 0) {
                R* p = static_cast<R*>(slab) + (int64_t)U.slot * KP + lig * 4;
#pragma unroll
                for (int t = 0; t < 4; ++t) p[t] = acc[t];
            }
            continue;
        }
        const double cross = sp_hals_row<KP, CROSS, R, SOLVE>(gs, inv, live, acc, Own + (int64_t)U.row * KP, k, sweeps, lig, grp, tol,
                                                              SOLVE ? counts + U.row : nullptr);
        if (lane == 0) objacc += cross;
    }
    if constexpr (CROSS) sp_hals_block_partial(objacc, ob, obj_part + blockIdx.x);
}

// Rows split into pieces: the pieces' partial r added in piece order (every group adds all of them: the same bits), then the
// sweep of a whole row; CROSS: the long columns' <h_new, r> into this launch's own slots obj_part[blockIdx.x].
template <int KP, bool CROSS, bool SOLVE = false>
__global__ __launch_bounds__(64 * SP_WAVES) void sp_hals_fixup_kernel(
    const SpLong* __restrict__ longs, int64_t nlong, const void* __restrict__ slab, float* Own, const float* __restrict__ Gf,
    float diag_add, double* __restrict__ obj_part, int k, int sweeps, const int* flag, float tol = 0.f,
    int32_t* __restrict__ counts = nullptr)
{
    if (*flag) return;
    constexpr int G = KP / 4;
    using R = typename std::conditional<CROSS, double, float>::type;
    __shared__ __attribute__((aligned(16))) float gs[KP * KP];
    __shared__ double ob[SP_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lig = lane % G, grp = lane / G;
    sp_hals_stage<KP>(gs, Gf, diag_add, k);
    float inv[4]; bool live[4];
    sp_hals_diag<KP>(gs, k, lig, inv, live);
    double objacc = 0.0;
    for (int64_t l = (int64_t)blockIdx.x * SP_WAVES + wave; l < nlong; l += (int64_t)gridDim.x * SP_WAVES) {
        const SpLong L = longs[l];
        R acc[4] = {0, 0, 0, 0};
        for (int p = 0; p < L.npieces; ++p) {
            const R* s = static_cast<const R*>(slab) + (int64_t)(L.slot0 + p) * KP + lig * 4;
#pragma unroll
            for (int t = 0; t < 4; ++t) acc[t] += s[t];
        }
        const double cross = sp_hals_row<KP, CROSS, R, SOLVE>(gs, inv, live, acc, Own + (int64_t)L.row * KP, k, sweeps, lig, grp, tol,
                                                              SOLVE ? counts + L.row : nullptr);
        if (lane == 0) objacc += cross;
    }
    if constexpr (CROSS) sp_hals_block_partial(objacc, ob, obj_part + blockIdx.x);
}

// one half-step: side 0 the W phase (own W, gather H^T, Gram 1), side 1 the H phase (own H^T, gather W, Gram 0, CROSS).
// *nparts: the objective partials the H phase left in hals_part.  SOLVE: the fold-in solve (sweeps: its cap; tol; the counts
// into foldin_sweeps).
template <int KP, bool CROSS, bool SOLVE = false>
static int launch_hals_phase(nmfx_engine* E, float* Own, const float* Other, float diag_add, int sweeps, int* nparts, float tol = 0.f) {
    nmfx_sparse* S = E->sp;
    constexpr int side = CROSS ? 1 : 0;
    SpSide& sd = S->side[side];
    const int* flag = &E->state->flag;
    void* slab = CROSS ? (void*)sd.slab64 : (void*)sd.slab;
    int32_t* counts = SOLVE ? S->foldin_sweeps : nullptr;
    hipLaunchKernelGGL((sp_hals_phase_kernel<KP, CROSS, SOLVE>), dim3(sd.nblk), dim3(64 * SP_WAVES), 0, E->stream, (const SpUnit*)sd.units,
                       sd.nunits, (const int32_t*)sd.idx, (const float*)sd.val, Other, Own, (const float*)S->gf[1 - side], diag_add,
                       slab, S->hals_part, E->k, sweeps, flag, tol, counts);
    NMFX_HIP(hipGetLastError());
    int nb = 0;
    if (sd.nlong) {
        nb = (int)std::min<int64_t>(4 * E->ncu, (sd.nlong + SP_WAVES - 1) / SP_WAVES);
        hipLaunchKernelGGL((sp_hals_fixup_kernel<KP, CROSS, SOLVE>), dim3(nb), dim3(64 * SP_WAVES), 0, E->stream, (const SpLong*)sd.longs,
                           sd.nlong, (const void*)slab, Own, (const float*)S->gf[1 - side], diag_add, S->hals_part + sd.nblk, E->k,
                           sweeps, flag, tol, counts);
        NMFX_HIP(hipGetLastError());
    }
    if (nparts) *nparts = sd.nblk + nb;
    return NMFX_OK;
}

// Iteration j: W phase, stats(W), H phase, stats(H), then obj[j + 1] of the new pair and the stop rule for loop index j.
// Two passes over the non-zeros.  Once the rule has fired every later launch returns at once: the pair stays the one the
// last recorded objective belongs to.
template <int KP>
static int sp_hals_iteration(nmfx_engine* E, double lw, double lh, int sweeps, int64_t min_iter, double tol1, double tol2, int64_t j) {
    nmfx_sparse* S = E->sp;
    const int* flag = &E->state->flag;
    float* W = E->W[0];
    int rc, nparts = 0;
    { ProfScope ps(E, "sp_hals_wphase");
      if ((rc = launch_hals_phase<KP, false>(E, W, S->Ht, (float)(2.0 * lw), sweeps, nullptr))) return rc; }
    { ProfScope ps(E, "sp_stats");
      if ((rc = launch_stats<KP>(E, W, E->m, 0, flag))) return rc; }
    { ProfScope ps(E, "sp_hals_hphase");
      if ((rc = launch_hals_phase<KP, true>(E, S->Ht, W, (float)(2.0 * lh), sweeps, &nparts))) return rc; }
    { ProfScope ps(E, "sp_stats");
      if ((rc = launch_stats<KP>(E, S->Ht, E->n, 1, flag))) return rc; }
    hipLaunchKernelGGL((sp_objective_kernel<false, false>), dim3(1), dim3(256), 0, E->stream, (const double*)S->hals_part, nparts,
                       (const double*)S->g64[0], (const double*)S->g64[1], (const double*)S->cs64[0], (const double*)S->cs64[1],
                       E->kp, S->x2, E->xf64, 1, (long long)(j + 1), (long long)min_iter, tol1, tol2, E->state, E->obj_hist);
    NMFX_HIP(hipGetLastError());
    return NMFX_OK;
}

// what both entry points refuse, nothing launched; then the guard (family HALS: on a sparse handle neither MUR nor HALS
// continues the other's run without nmfx_set_factors) and the buffers of first use
// wide: the kp = 256 pair (nmfx_hals_sparse_wide_*), which also needs the buffers of the right-hand sides
static int sp_hals_ready(nmfx_engine* E, const char* who, int sweeps, double lw, double lh, int64_t first, int64_t count, bool wide = false) {
    if (!E) return NMFX_E_ARG;
    if (!E->sp) { E->err = std::string(who) + ": needs a sparse handle (nmfx_create_csr); a dense handle runs nmfx_hals_run"; return NMFX_E_ARG; }
    if (E->sp->masked) { E->err = std::string(who) + ": not available on a masked handle (nmfx_set_masked): masked handles run MUR only"; return NMFX_E_ARG; }
    if (!wide && E->kp > 128) { E->err = nmfx_small_k_text(who); return NMFX_E_ARG; }
    if (wide && E->kp != 256) { E->err = std::string(who) + ": serves 129 <= k <= 256 components (kp = 256); nmfx_hals_sparse_run serves k <= 128"; return NMFX_E_ARG; }
    nmfx_entry a = {NMFX_FAM_HALS, first, count, NMFX_D_NONE, NMFX_D_NONE};
    a.bad = nmfx_hals_args_bad(who, sweeps, first, count, &lw, &lh);
    int rc = nmfx_enter(E, a); if (rc) return rc;
    E->run.in_place();
    nmfx_sparse* S = E->sp;
    if ((rc = nmfx_lazy_alloc(E, &S->hals_part, (int64_t)8 * E->ncu + 64))) return rc;
    if ((rc = nmfx_lazy_alloc(E, &S->side[1].slab64, std::max<int64_t>(1, S->side[1].npieces * E->kp)))) return rc;
    if (!wide) return NMFX_OK;
    if ((rc = nmfx_lazy_alloc(E, &S->hals_r32, std::max<int64_t>(1, std::max(E->m, E->n) * E->kp)))) return rc;
    return nmfx_lazy_alloc(E, &S->hals_r64, std::max<int64_t>(1, E->n * E->kp));
}

extern "C" int nmfx_hals_sparse_run(nmfx_handle_t E, double lambda_w, double lambda_h, int sweeps, int64_t min_iter, double tol1,
                                    double tol2, int64_t first, int64_t count) {
    int rc = sp_hals_ready(E, "nmfx_hals_sparse_run", sweeps, lambda_w, lambda_h, first, count); if (rc) return rc;
    if (first == 0 && count > 0) {                     // obj[0]: one objective-only pass over the start
        if ((rc = objective_pass(E, NMFX_EU, E->W[0], &E->state->flag))) return rc;
        if ((rc = launch_objective(E, NMFX_EU, E->xf64, true, 0, min_iter, tol1, tol2))) return rc;
    }
    for (int64_t j = first; j < first + count && !rc; ++j) {
#define SP_IT(KP) sp_hals_iteration<KP>(E, lambda_w, lambda_h, sweeps, min_iter, tol1, tol2, j)
        switch (E->kp) { case 4: rc = SP_IT(4); break; case 8: rc = SP_IT(8); break; case 16: rc = SP_IT(16); break;
                         case 32: rc = SP_IT(32); break; case 64: rc = SP_IT(64); break; default: rc = SP_IT(128); break; }
#undef SP_IT
    }
    return rc;
}

// Every iteration has recorded the objective of the pair it left: there is something to record only where obj[iters_done]
// does not exist yet (no iteration has run).
extern "C" int nmfx_hals_sparse_finish(nmfx_handle_t E, int64_t min_iter, double tol1, double tol2, int64_t iters_done) {
    int rc = sp_hals_ready(E, "nmfx_hals_sparse_finish", 1, 0.0, 0.0, iters_done, 0); if (rc) return rc;
    DevState hs;
    NMFX_HIP(hipMemcpyAsync(&hs, E->state, sizeof(DevState), hipMemcpyDeviceToHost, E->stream));
    NMFX_HIP(hipStreamSynchronize(E->stream));
    if (hs.flag || hs.n_obj > iters_done) return NMFX_OK;
    if ((rc = objective_pass(E, NMFX_EU, E->W[0], &E->state->flag))) return rc;
    return launch_objective(E, NMFX_EU, E->xf64, true, iters_done, min_iter, tol1, tol2);
}

// ---------------------------------------------------------------------------------------------------------------------
// HALS on sparse V with 129 .. 256 components (nmfx_hals_sparse_wide_run)
// ---------------------------------------------------------------------------------------------------------------------
// At kp = 256 the copy of G the sweep of sp_hals_phase_kernel reads is 256 KiB: it no longer fits in LDS.  The half-step is
// composed instead: a gather launch leaves every owned row's r in a buffer, [rows][256], and nmfx_hals_wide_sweep (kernels_hals.hip)
// sweeps the rows on G streamed through LDS in row tiles -- the owned factor is row-major along its long dimension, which is
// the sweep's W layout on both sides (sj = 1, sc = 256).
//
// The gather is sp_hals_gather at KP = 256: a wave holds a 256-vector as one float4 per lane, so a group is the whole wave
// (NG = 1) and each non-zero costs one coalesced 1 KiB row of the other factor, four of them in flight.  The wave index is made
// uniform (v_readfirstlane), so the unit, and with it the index and the value of every non-zero, is read with scalar loads:
// one request per non-zero where a vector load would issue 64 lanes for the same address.  Pieces of rows longer than SP_CHUNK
// go to the slab and sp_hals_wide_fixup_kernel adds them in piece order, as sp_hals_fixup_kernel does.
//
// CROSS (the H phase): r is summed in f64, stored in f64 (r64) and rounded to f32 (r32) for the sweep only; after the sweep
// sp_hals_wide_cross_kernel sums <h_new_c, r64_c> per block in a fixed order -- the cross term of the objective.
template <bool CROSS>
__device__ __forceinline__ void sp_hals_wide_store(const typename std::conditional<CROSS, double, float>::type (&acc)[4], int64_t row,
                                                   float* __restrict__ r32, double* __restrict__ r64, int lane)
{
    *reinterpret_cast<float4*>(r32 + row * 256 + lane * 4) = make_float4((float)acc[0], (float)acc[1], (float)acc[2], (float)acc[3]);
    if constexpr (CROSS) {
        double* p = r64 + row * 256 + lane * 4;
        *reinterpret_cast<double2*>(p) = make_double2(acc[0], acc[1]);
        *reinterpret_cast<double2*>(p + 2) = make_double2(acc[2], acc[3]);
    }
}

template <bool CROSS>
__global__ __launch_bounds__(64 * SP_WAVES) void sp_hals_wide_gather_kernel(
    const SpUnit* __restrict__ units, int64_t nunits, const int32_t* __restrict__ idx, const float* __restrict__ val,
    const float* __restrict__ Other, void* __restrict__ slab, float* __restrict__ r32, double* __restrict__ r64, const int* flag)
{
    if (*flag) return;
    using R = typename std::conditional<CROSS, double, float>::type;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (int64_t u = (int64_t)blockIdx.x * SP_WAVES + wave; u < nunits; u += (int64_t)gridDim.x * SP_WAVES) {
        const SpUnit U = units[u];
        R acc[4] = {0, 0, 0, 0};
        sp_hals_gather<256, CROSS>(U.beg, U.len, idx, val, Other, lane, 0, acc);
        if (U.slot >= 0) {
            R* p = static_cast<R*>(slab) + (int64_t)U.slot * 256 + lane * 4;
#pragma unroll
            for (int t = 0; t < 4; ++t) p[t] = acc[t];
        } else {
            sp_hals_wide_store<CROSS>(acc, U.row, r32, r64, lane);
        }
    }
}

template <bool CROSS>
__global__ __launch_bounds__(64 * SP_WAVES) void sp_hals_wide_fixup_kernel(
    const SpLong* __restrict__ longs, int64_t nlong, const void* __restrict__ slab, float* __restrict__ r32, double* __restrict__ r64,
    const int* flag)
{
    if (*flag) return;
    using R = typename std::conditional<CROSS, double, float>::type;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int64_t l = (int64_t)blockIdx.x * SP_WAVES + wave; l < nlong; l += (int64_t)gridDim.x * SP_WAVES) {
        const SpLong L = longs[l];
        R acc[4] = {0, 0, 0, 0};
        for (int p = 0; p < L.npieces; ++p) {
            const R* s = static_cast<const R*>(slab) + (int64_t)(L.slot0 + p) * 256 + lane * 4;
#pragma unroll
            for (int t = 0; t < 4; ++t) acc[t] += s[t];
        }
        sp_hals_wide_store<CROSS>(acc, L.row, r32, r64, lane);
    }
}

// Sum_c <x_c, r64_c> over the rows c of X [rows][256]: a wave per row (the row's sum as sp_hals_row forms it, then a fixed
// butterfly), the waves' rows in a fixed stride, the block's partial into part[blockIdx.x].
__global__ __launch_bounds__(64 * SP_WAVES) void sp_hals_wide_cross_kernel(const float* __restrict__ X, const double* __restrict__ r64,
                                                                          int64_t rows, double* __restrict__ part, const int* flag)
{
    if (*flag) return;
    __shared__ double ob[SP_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double objacc = 0.0;
    for (int64_t c = (int64_t)blockIdx.x * SP_WAVES + wave; c < rows; c += (int64_t)gridDim.x * SP_WAVES) {
        const float4 x = *reinterpret_cast<const float4*>(X + c * 256 + lane * 4);
        const double2 ra = *reinterpret_cast<const double2*>(r64 + c * 256 + lane * 4);
        const double2 rb = *reinterpret_cast<const double2*>(r64 + c * 256 + lane * 4 + 2);
        double cross = fma((double)x.x, ra.x, fma((double)x.y, ra.y, fma((double)x.z, rb.x, (double)x.w * rb.y)));
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) cross += __shfl_xor(cross, off, 64);
        if (lane == 0) objacc += cross;
    }
    sp_hals_block_partial(objacc, ob, part + blockIdx.x);
}

// the right-hand sides of one half-step into hals_r32 (CROSS: and hals_r64): side 0 gathers H^T over the CSR rows, side 1
// (CROSS) the new W over the CSC columns
template <bool CROSS>
static int launch_hals_wide_gather(nmfx_engine* E, const float* Other) {
    nmfx_sparse* S = E->sp;
    SpSide& sd = S->side[CROSS ? 1 : 0];
    const int* flag = &E->state->flag;
    void* slab = CROSS ? (void*)sd.slab64 : (void*)sd.slab;
    hipLaunchKernelGGL((sp_hals_wide_gather_kernel<CROSS>), dim3(sd.nblk), dim3(64 * SP_WAVES), 0, E->stream, (const SpUnit*)sd.units,
                       sd.nunits, (const int32_t*)sd.idx, (const float*)sd.val, Other, slab, S->hals_r32, S->hals_r64, flag);
    NMFX_HIP(hipGetLastError());
    if (sd.nlong) {
        const int nb = (int)std::min<int64_t>(4 * E->ncu, (sd.nlong + SP_WAVES - 1) / SP_WAVES);
        hipLaunchKernelGGL((sp_hals_wide_fixup_kernel<CROSS>), dim3(nb), dim3(64 * SP_WAVES), 0, E->stream, (const SpLong*)sd.longs,
                           sd.nlong, (const void*)slab, S->hals_r32, S->hals_r64, flag);
        NMFX_HIP(hipGetLastError());
    }
    return NMFX_OK;
}

// Iteration j, the launches of sp_hals_iteration with each half-step in two: gather, then the tiled sweep.
static int sp_hals_wide_iteration(nmfx_engine* E, double lw, double lh, int sweeps, int64_t min_iter, double tol1, double tol2, int64_t j) {
    nmfx_sparse* S = E->sp;
    const int* flag = &E->state->flag;
    float* W = E->W[0];
    int rc;
    { ProfScope ps(E, "sp_hals_wide_wgather");
      if ((rc = launch_hals_wide_gather<false>(E, S->Ht))) return rc; }
    { ProfScope ps(E, "sp_hals_wide_wsweep");
      if ((rc = nmfx_hals_wide_sweep(E, S->gf[1], (float)(2.0 * lw), S->hals_r32, W, 1, 256, E->m, sweeps))) return rc; }
    { ProfScope ps(E, "sp_stats");
      if ((rc = launch_stats<256>(E, W, E->m, 0, flag))) return rc; }
    { ProfScope ps(E, "sp_hals_wide_hgather");
      if ((rc = launch_hals_wide_gather<true>(E, W))) return rc; }
    { ProfScope ps(E, "sp_hals_wide_hsweep");
      if ((rc = nmfx_hals_wide_sweep(E, S->gf[0], (float)(2.0 * lh), S->hals_r32, S->Ht, 1, 256, E->n, sweeps))) return rc; }
    const int nparts = (int)std::max<int64_t>(1, std::min<int64_t>(4 * E->ncu, (E->n + SP_WAVES - 1) / SP_WAVES));
    { ProfScope ps(E, "sp_hals_wide_cross");
      hipLaunchKernelGGL(sp_hals_wide_cross_kernel, dim3(nparts), dim3(64 * SP_WAVES), 0, E->stream, (const float*)S->Ht,
                         (const double*)S->hals_r64, E->n, S->hals_part, flag);
      NMFX_HIP(hipGetLastError()); }
    { ProfScope ps(E, "sp_stats");
      if ((rc = launch_stats<256>(E, S->Ht, E->n, 1, flag))) return rc; }
    hipLaunchKernelGGL((sp_objective_kernel<false, false>), dim3(1), dim3(256), 0, E->stream, (const double*)S->hals_part, nparts,
                       (const double*)S->g64[0], (const double*)S->g64[1], (const double*)S->cs64[0], (const double*)S->cs64[1],
                       E->kp, S->x2, E->xf64, 1, (long long)(j + 1), (long long)min_iter, tol1, tol2, E->state, E->obj_hist);
    NMFX_HIP(hipGetLastError());
    return NMFX_OK;
}

extern "C" int nmfx_hals_sparse_wide_run(nmfx_handle_t E, double lambda_w, double lambda_h, int sweeps, int64_t min_iter, double tol1,
                                         double tol2, int64_t first, int64_t count) {
    int rc = sp_hals_ready(E, "nmfx_hals_sparse_wide_run", sweeps, lambda_w, lambda_h, first, count, true); if (rc) return rc;
    if (first == 0 && count > 0) {                     // obj[0]: one objective-only pass over the start
        if ((rc = objective_pass(E, NMFX_EU, E->W[0], &E->state->flag))) return rc;
        if ((rc = launch_objective(E, NMFX_EU, E->xf64, true, 0, min_iter, tol1, tol2))) return rc;
    }
    for (int64_t j = first; j < first + count && !rc; ++j)
        rc = sp_hals_wide_iteration(E, lambda_w, lambda_h, sweeps, min_iter, tol1, tol2, j);
    return rc;
}

// as nmfx_hals_sparse_finish
extern "C" int nmfx_hals_sparse_wide_finish(nmfx_handle_t E, int64_t min_iter, double tol1, double tol2, int64_t iters_done) {
    int rc = sp_hals_ready(E, "nmfx_hals_sparse_wide_finish", 1, 0.0, 0.0, iters_done, 0, true); if (rc) return rc;
    DevState hs;
    NMFX_HIP(hipMemcpyAsync(&hs, E->state, sizeof(DevState), hipMemcpyDeviceToHost, E->stream));
    NMFX_HIP(hipStreamSynchronize(E->stream));
    if (hs.flag || hs.n_obj > iters_done) return NMFX_OK;
    if ((rc = objective_pass(E, NMFX_EU, E->W[0], &E->state->flag))) return rc;
    return launch_objective(E, NMFX_EU, E->xf64, true, iters_done, min_iter, tol1, tol2);
}

// ---------------------------------------------------------------------------------------------------------------------
// HALS on a masked handle (nmfx_hals_masked_run)
// ---------------------------------------------------------------------------------------------------------------------
// With entries missing the owned rows no longer share one Gram matrix: row i of W sees only the columns observed in that row,
//     G = Sum_{e in Omega} f_e f_e^T + 2 lambda I,    r = Sum_{e in Omega} v_e f_e      (f_e: the gathered row of the other factor)
// and a half-step is the sweep of sp_hals_row on every row's own (G, r).  One wave forms G on the f32 MFMA pipe
// (v_mfma_f32_16x16x4_f32, exact f32): a step takes four observed entries, lane l holds NB = max(1, KP / 16) consecutive
// components NB (l & 15) + b of entry l >> 4 (one load of NB floats), and operand b against operand b' accumulates the 16 x 16
// block of G whose rows are the components NB i + b and columns NB j + b' -- a permutation of G that is undone when the block
// is written to LDS.  Only b <= b' is computed (NB (NB + 1) / 2 accumulators of 4 VGPRs: 10 at KP = 64) and mirrored on the
// way out; the diagonal blocks are symmetric bit for bit (the same products in the same order).  KP = 4 and 8 use one block
// with the lanes past KP holding zeros.  A slot past the row's end holds zero operands (not only a zero value).  r is summed
// with plain FMAs next to it, per entry slot, and the four slots are added by a fixed butterfly.
//
// G (then 2 lambda on the diagonal of the first k components, in f32) and r go to a wave-private LDS region of KP x KP + KP
// floats and the wave runs the sweep of sparse HALS on it, unchanged.  The unit loop has a different trip count per wave, so
// there is no block barrier in it: the hand-off between the lanes of one wave is ordered by a wavefront-scope fence.
//
// Rows longer than a piece (SP_CHUNK entries): the phase kernel skips piece units, and sp_mhals_long_kernel takes one
// workgroup per long row (a blockIdx-strided loop: block-uniform, so block barriers are legal there).  Wave w sums the pieces
// w, w + MW, ... in registers and writes its [G | r] to an LDS region of its own; the block adds the regions in wave order,
// and wave 0 sweeps.  No slab of k^2 floats per piece, no atomics: two runs give the same bits.
template <int KP> struct MhCfg {
    static constexpr int NB = KP >= 16 ? KP / 16 : 1;          // 16-wide operand blocks
    static constexpr int NACC = NB * (NB + 1) / 2;             // blocks on and above the diagonal
    static constexpr int MW = KP >= 64 ? 4 : 8;                // waves per block: (KP^2 + KP) floats of LDS each (65 KiB at KP = 64)
    static constexpr int REGION = KP * KP + KP;                // [G | r]
};
typedef float mh_f4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ void mh_wave_fence() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// [G | r] of the entries [beg, beg + len) of one row, added to acc / racc (this lane's share: the header).  Blocks of 16
// entries (four MFMA steps), software-pipelined: while block b is multiplied, the rows of block b + 1 and the indices and
// values of block b + 2 are in flight (a gather is two dependent loads, and 40 MFMAs do not cover both).
template <int KP>
__device__ __forceinline__ void mh_accumulate(long long beg, int len, const int32_t* __restrict__ idx, const float* __restrict__ val,
                                              const float* __restrict__ Other, mh_f4 (&acc)[MhCfg<KP>::NACC], float (&racc)[MhCfg<KP>::NB], int lane)
{
    constexpr int NB = MhCfg<KP>::NB;
    const int slot = lane >> 4, c0 = NB * (lane & 15);
    const bool holds = c0 < KP;                                 // (KP = 4, 8: the lanes past KP hold zeros)
    const long long end = beg + len;
    if (len <= 0) return;
    // indices and values of the block at e0; a slot past the end reads nothing: row 0 with value 0
    auto load_cx = [&](long long e0, int (&c)[4], float (&x)[4]) {
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const long long e = e0 + 4 * t + slot;
            const bool ok = e < end;
            c[t] = ok ? idx[e] : 0;
            x[t] = ok ? val[e] : 0.f;
        }
    };
    auto load_f = [&](const int (&c)[4], float (&f)[4][NB]) {
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const float* src = Other + (int64_t)c[t] * KP + (holds ? c0 : 0);
            if constexpr (NB == 4) {
                const float4 v = *reinterpret_cast<const float4*>(src);
                f[t][0] = v.x; f[t][1] = v.y; f[t][2] = v.z; f[t][3] = v.w;
            } else if constexpr (NB == 2) {
                const float2 v = *reinterpret_cast<const float2*>(src);
                f[t][0] = v.x; f[t][1] = v.y;
            } else {
                f[t][0] = *src;
            }
        }
    };
    auto multiply = [&](long long e0, float (&f)[4][NB], const float (&x)[4]) {
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const bool ok = e0 + 4 * t + slot < end;
#pragma unroll
            for (int b = 0; b < NB; ++b) {
                f[t][b] = (ok && holds) ? f[t][b] : 0.f;        // a slot past the end gathered row 0: a zero operand
                racc[b] = fmaf(x[t], f[t][b], racc[b]);
            }
            int a = 0;
#pragma unroll
            for (int ba = 0; ba < NB; ++ba) {
#pragma unroll
                for (int bb = ba; bb < NB; ++bb, ++a) acc[a] = __builtin_amdgcn_mfma_f32_16x16x4f32(f[t][ba], f[t][bb], acc[a], 0, 0, 0);
            }
        }
    };
    int cA[4], cB[4], cC[4], cD[4]; float xA[4], xB[4], xC[4], xD[4]; float fA[4][NB], fB[4][NB];
    load_cx(beg, cA, xA);
    load_f(cA, fA);
    load_cx(beg + 16, cB, xB);
    for (long long e0 = beg; e0 < end; e0 += 32) {             // (wave-uniform bounds)
        load_f(cB, fB);
        load_cx(e0 + 32, cC, xC);
        multiply(e0, fA, xA);
        if (e0 + 16 >= end) break;
        load_f(cC, fA);
        load_cx(e0 + 48, cD, xD);
        multiply(e0 + 16, fB, xB);
#pragma unroll
        for (int t = 0; t < 4; ++t) { xA[t] = xC[t]; cB[t] = cD[t]; xB[t] = xD[t]; }
    }
}

// This lane's share of [G | r] into the LDS region, mirrored; r after the butterfly over the four entry slots.  Every element
// of the region is written by exactly one lane.
template <int KP>
__device__ __forceinline__ void mh_deposit(float* gs, const mh_f4 (&acc)[MhCfg<KP>::NACC], const float (&racc)[MhCfg<KP>::NB], int lane) {
    constexpr int NB = MhCfg<KP>::NB;
    const int j = lane & 15, i0 = 4 * (lane >> 4);
    int a = 0;
#pragma unroll
    for (int ba = 0; ba < NB; ++ba) {
#pragma unroll
        for (int bb = ba; bb < NB; ++bb, ++a) {
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int row = NB * (i0 + v) + ba, col = NB * j + bb;
                if (row < KP && col < KP) {
                    const float g = acc[a][v];
                    gs[row * KP + col] = g;
                    if (ba != bb) gs[col * KP + row] = g;
                }
            }
        }
    }
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        float r = racc[b];
        r += __shfl_xor(r, 16, 64);
        r += __shfl_xor(r, 32, 64);
        const int c = NB * j + b;
        if (lane < 16 && c < KP) gs[KP * KP + c] = r;
    }
}

// The region holds the row's summed [G | r]: 2 lambda on the diagonal of the first k components, then the sweep of sparse
// HALS from the row's current values; group 0 writes the row in place.  Called by every lane of ONE wave.
// SOLVE (fold-in): the solve of sp_hals_row on the region, whose r (at gs + KP KP) stays in place for the refresh; the count to *count.
template <int KP, bool SOLVE = false>
__device__ __forceinline__ void mh_sweep_row(float* gs, float diag_add, float* row, int k, int sweeps, int lane, float tol = 0.f,
                                             int32_t* count = nullptr) {
    constexpr int G = KP / 4;
    const int lig = lane % G, grp = lane / G;
    mh_wave_fence();
    if (lane < k) gs[lane * KP + lane] += diag_add;             // (k <= KP <= 64)
    mh_wave_fence();
    float inv[4]; bool live[4];
    sp_hals_diag<KP>(gs, k, lig, inv, live);
    const float4 r4 = *reinterpret_cast<const float4*>(gs + KP * KP + lig * 4);
    const float r[4] = {r4.x, r4.y, r4.z, r4.w};
    sp_hals_row<KP, false, float, SOLVE>(gs, inv, live, r, row, k, sweeps, lig, grp, tol, count, SOLVE ? gs + KP * KP : nullptr);
    mh_wave_fence();                                            // (the next row's [G | r] overwrites the region)
}

//   Own [rows][KP]: the factor being updated, in place (a row is owned by one wave; the gathers read the other factor only);
//   Other [*][KP]: the factor gathered per observed entry; diag_add = (float)(2 lambda).
//   SOLVE (fold-in): each row's [G | r] is formed once and swept in place to the stop rule (tol; `sweeps` is the cap); its count to counts[row].
template <int KP, bool SOLVE = false>
__global__ __launch_bounds__(64 * MhCfg<KP>::MW) void sp_mhals_phase_kernel(
    const SpUnit* __restrict__ units, int64_t nunits, const int32_t* __restrict__ idx, const float* __restrict__ val,
    const float* __restrict__ Other, float* Own, float diag_add, int k, int sweeps, const int* flag, float tol = 0.f,
    int32_t* __restrict__ counts = nullptr)
{
    if (*flag) return;
    constexpr int MW = MhCfg<KP>::MW, NB = MhCfg<KP>::NB, NACC = MhCfg<KP>::NACC;
    __shared__ __attribute__((aligned(16))) float lds[MW * MhCfg<KP>::REGION];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float* gs = lds + wave * MhCfg<KP>::REGION;
    for (int64_t u = (int64_t)blockIdx.x * MW + wave; u < nunits; u += (int64_t)gridDim.x * MW) {      // (no block barrier in here)
        const SpUnit U = units[u];
        if (U.slot >= 0) continue;                              // a piece of a long row: sp_mhals_long_kernel (wave-uniform)
        mh_f4 acc[NACC]; float racc[NB];
#pragma unroll
        for (int a = 0; a < NACC; ++a) acc[a] = mh_f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int b = 0; b < NB; ++b) racc[b] = 0.f;
        mh_accumulate<KP>(U.beg, U.len, idx, val, Other, acc, racc, lane);
        mh_deposit<KP>(gs, acc, racc, lane);
        mh_sweep_row<KP, SOLVE>(gs, diag_add, Own + (int64_t)U.row * KP, k, sweeps, lane, tol, SOLVE ? counts + U.row : nullptr);
    }
}

// One workgroup per long row; the pieces of row l are the units [unit0, unit0 + npieces).
template <int KP, bool SOLVE = false>
__global__ __launch_bounds__(64 * MhCfg<KP>::MW) void sp_mhals_long_kernel(
    const SpLong* __restrict__ longs, int64_t nlong, const SpUnit* __restrict__ units, const int32_t* __restrict__ idx,
    const float* __restrict__ val, const float* __restrict__ Other, float* Own, float diag_add, int k, int sweeps, const int* flag,
    float tol = 0.f, int32_t* __restrict__ counts = nullptr)
{
    if (*flag) return;
    constexpr int MW = MhCfg<KP>::MW, NB = MhCfg<KP>::NB, NACC = MhCfg<KP>::NACC;
    constexpr int REGION = MhCfg<KP>::REGION;
    __shared__ __attribute__((aligned(16))) float gs[MW * REGION];      // region w: wave w's partial [G | r]; their sum lands in region 0
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int64_t l = blockIdx.x; l < nlong; l += gridDim.x) {   // (block-uniform: the barriers below are reached by every wave)
        const SpLong L = longs[l];
        mh_f4 acc[NACC]; float racc[NB];
#pragma unroll
        for (int a = 0; a < NACC; ++a) acc[a] = mh_f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int b = 0; b < NB; ++b) racc[b] = 0.f;
        for (int p = wave; p < L.npieces; p += MW) {
            const SpUnit U = units[(int64_t)L.unit0 + p];
            mh_accumulate<KP>(U.beg, U.len, idx, val, Other, acc, racc, lane);
        }
        mh_deposit<KP>(gs + wave * REGION, acc, racc, lane);
        __syncthreads();
        for (int i = threadIdx.x; i < REGION; i += 64 * MW) {   // the waves' partial sums, added in wave order
            float sum = gs[i];
#pragma unroll
            for (int w = 1; w < MW; ++w) sum += gs[w * REGION + i];
            gs[i] = sum;
        }
        __syncthreads();
        if (wave == 0) mh_sweep_row<KP, SOLVE>(gs, diag_add, Own + (int64_t)L.row * KP, k, sweeps, lane, tol, SOLVE ? counts + L.row : nullptr);
        __syncthreads();                                        // (the next row's deposit overwrites the region)
    }
}

// one half-step: side 0 the W phase (own W, gather H^T), side 1 the H phase (own H^T, gather W)
// SOLVE: the fold-in solve (sweeps: its cap; tol; the counts into foldin_sweeps)
template <int KP, bool SOLVE = false>
static int launch_mhals_phase(nmfx_engine* E, int side, float* Own, const float* Other, float diag_add, int sweeps, float tol = 0.f) {
    SpSide& sd = E->sp->side[side];
    constexpr int MW = MhCfg<KP>::MW;
    const int* flag = &E->state->flag;
    int32_t* counts = SOLVE ? E->sp->foldin_sweeps : nullptr;
    const int nb = (int)std::max<int64_t>(1, std::min<int64_t>((int64_t)(32 / MW) * E->ncu, (sd.nunits + MW - 1) / MW));
    hipLaunchKernelGGL((sp_mhals_phase_kernel<KP, SOLVE>), dim3(nb), dim3(64 * MW), 0, E->stream, (const SpUnit*)sd.units, sd.nunits,
                       (const int32_t*)sd.idx, (const float*)sd.val, Other, Own, diag_add, E->k, sweeps, flag, tol, counts);
    NMFX_HIP(hipGetLastError());
    if (sd.nlong) {
        const int nl = (int)std::min<int64_t>(4 * E->ncu, sd.nlong);
        hipLaunchKernelGGL((sp_mhals_long_kernel<KP, SOLVE>), dim3(nl), dim3(64 * MW), 0, E->stream, (const SpLong*)sd.longs, sd.nlong,
                           (const SpUnit*)sd.units, (const int32_t*)sd.idx, (const float*)sd.val, Other, Own, diag_add, E->k, sweeps, flag,
                           tol, counts);
        NMFX_HIP(hipGetLastError());
    }
    return NMFX_OK;
}

// Iteration j: W phase, H phase, the masked objective pass over the observed entries (f64 per entry), then obj[j + 1] of the
// new pair and the stop rule for loop index j.  No Gram and no stats passes.  Once the rule has fired every launch returns at once.
template <int KP>
static int sp_mhals_iteration(nmfx_engine* E, double lw, double lh, int sweeps, int64_t min_iter, double tol1, double tol2, int64_t j) {
    nmfx_sparse* S = E->sp;
    float* W = E->W[0];
    int rc;
    { ProfScope ps(E, "sp_mhals_wphase");
      if ((rc = launch_mhals_phase<KP>(E, 0, W, S->Ht, (float)(2.0 * lw), sweeps))) return rc; }
    { ProfScope ps(E, "sp_mhals_hphase");
      if ((rc = launch_mhals_phase<KP>(E, 1, S->Ht, W, (float)(2.0 * lh), sweeps))) return rc; }
    { ProfScope ps(E, "sp_mhals_objective");
      if ((rc = sp_objective_pass<KP>(E, NMFX_EU, W, &E->state->flag))) return rc;
      if ((rc = launch_objective(E, NMFX_EU, E->xf64, true, j + 1, min_iter, tol1, tol2))) return rc; }
    return NMFX_OK;
}

// what both entry points refuse, nothing launched; then the guard (family HALS)
static int sp_mhals_ready(nmfx_engine* E, const char* who, int sweeps, double lw, double lh, int64_t first, int64_t count) {
    if (!E) return NMFX_E_ARG;
    if (!E->sp) { E->err = std::string(who) + ": needs a sparse handle (nmfx_create_csr) made masked (nmfx_set_masked)"; return NMFX_E_ARG; }
    if (!E->sp->masked) { E->err = std::string(who) + ": needs a masked handle (nmfx_set_masked); an unmasked sparse handle runs nmfx_hals_sparse_run"; return NMFX_E_ARG; }
    if (E->kp > 64) { E->err = std::string(who) + ": not available with more than 64 components in this build"; return NMFX_E_ARG; }
    nmfx_entry a = {NMFX_FAM_HALS, first, count, NMFX_D_NONE, NMFX_D_NONE};
    a.bad = nmfx_hals_args_bad(who, sweeps, first, count, &lw, &lh);
    int rc = nmfx_enter(E, a); if (rc) return rc;
    E->run.in_place();
    return NMFX_OK;
}

extern "C" int nmfx_hals_masked_run(nmfx_handle_t E, double lambda_w, double lambda_h, int sweeps, int64_t min_iter, double tol1,
                                    double tol2, int64_t first, int64_t count) {
    int rc = sp_mhals_ready(E, "nmfx_hals_masked_run", sweeps, lambda_w, lambda_h, first, count); if (rc) return rc;
    if (first == 0 && count > 0) {                     // obj[0]: one objective-only pass over the start
        if ((rc = objective_pass(E, NMFX_EU, E->W[0], &E->state->flag))) return rc;
        if ((rc = launch_objective(E, NMFX_EU, E->xf64, true, 0, min_iter, tol1, tol2))) return rc;
    }
    for (int64_t j = first; j < first + count && !rc; ++j) {
#define SP_IT(KP) sp_mhals_iteration<KP>(E, lambda_w, lambda_h, sweeps, min_iter, tol1, tol2, j)
        switch (E->kp) { case 4: rc = SP_IT(4); break; case 8: rc = SP_IT(8); break; case 16: rc = SP_IT(16); break;
                         case 32: rc = SP_IT(32); break; default: rc = SP_IT(64); break; }
#undef SP_IT
    }
    return rc;
}

// as nmfx_hals_sparse_finish: something to record only where obj[iters_done] does not exist yet
extern "C" int nmfx_hals_masked_finish(nmfx_handle_t E, int64_t min_iter, double tol1, double tol2, int64_t iters_done) {
    int rc = sp_mhals_ready(E, "nmfx_hals_masked_finish", 1, 0.0, 0.0, iters_done, 0); if (rc) return rc;
    DevState hs;
    NMFX_HIP(hipMemcpyAsync(&hs, E->state, sizeof(DevState), hipMemcpyDeviceToHost, E->stream));
    NMFX_HIP(hipStreamSynchronize(E->stream));
    if (hs.flag || hs.n_obj > iters_done) return NMFX_OK;
    if ((rc = objective_pass(E, NMFX_EU, E->W[0], &E->state->flag))) return rc;
    return launch_objective(E, NMFX_EU, E->xf64, true, iters_done, min_iter, tol1, tol2);
}

// ---------------------------------------------------------------------------------------------------------------------
// HALS fold-in (nmfx_hals_foldin_run)
// ---------------------------------------------------------------------------------------------------------------------
// H for the handle's V against the W that was set, W never touched.  With W fixed a column's system depends on V and W only:
// the H-side kernels of the two families above form it once (one gather; on a masked handle the column's own Gram) and
// sp_hals_sweeps<SOLVE> sweeps it in place until the column's stop rule or the cap.  obj[0] is the start's objective and obj[1] the
// result's, each as its family records it: an objective-only pass (both on a masked handle), and on an unmasked handle the
// solve's own Sum <h_c, r_c> with the Gram of the new H for obj[1].  The stop rule of the outer loop never fires here.
#define SP_FOLDIN_NEVER ((int64_t)1 << 40)

template <int KP>
static int sp_foldin_solve(nmfx_engine* E, double lh, float tol, int max_sweeps) {
    nmfx_sparse* S = E->sp;
    const int* flag = &E->state->flag;
    int rc, nparts = 0;
    { ProfScope ps(E, "sp_hals_foldin");
      if ((rc = launch_hals_phase<KP, true, true>(E, S->Ht, E->W[0], (float)(2.0 * lh), max_sweeps, &nparts, tol))) return rc; }
    { ProfScope ps(E, "sp_stats");
      if ((rc = launch_stats<KP>(E, S->Ht, E->n, 1, flag))) return rc; }
    hipLaunchKernelGGL((sp_objective_kernel<false, false>), dim3(1), dim3(256), 0, E->stream, (const double*)S->hals_part, nparts,
                       (const double*)S->g64[0], (const double*)S->g64[1], (const double*)S->cs64[0], (const double*)S->cs64[1],
                       E->kp, S->x2, E->xf64, 1, 1LL, (long long)SP_FOLDIN_NEVER, 0.0, 0.0, E->state, E->obj_hist);
    NMFX_HIP(hipGetLastError());
    return NMFX_OK;
}

template <int KP>
static int sp_mfoldin_solve(nmfx_engine* E, double lh, float tol, int max_sweeps) {
    int rc;
    { ProfScope ps(E, "sp_mhals_foldin");
      if ((rc = launch_mhals_phase<KP, true>(E, 1, E->sp->Ht, E->W[0], (float)(2.0 * lh), max_sweeps, tol))) return rc; }
    { ProfScope ps(E, "sp_mhals_objective");
      if ((rc = sp_objective_pass<KP>(E, NMFX_EU, E->W[0], &E->state->flag))) return rc;
      if ((rc = launch_objective(E, NMFX_EU, E->xf64, true, 1, SP_FOLDIN_NEVER, 0.0, 0.0))) return rc; }
    return NMFX_OK;
}

extern "C" int nmfx_hals_foldin_run(nmfx_handle_t E, double lambda_h, double tol, int max_sweeps) {
    const char* who = "nmfx_hals_foldin_run";
    if (!E) return NMFX_E_ARG;
    if (!E->sp) { E->err = std::string(who) + ": needs a sparse handle (nmfx_create_csr), masked or not; a dense handle runs nmfx_foldin_run"; return NMFX_E_ARG; }
    nmfx_sparse* S = E->sp;
    if (S->masked && E->kp > 64) { E->err = std::string(who) + ": not available on a masked handle with more than 64 components in this build"; return NMFX_E_ARG; }
    if (E->kp > 128) { E->err = nmfx_small_k_text(who); return NMFX_E_ARG; }
    nmfx_entry a = {NMFX_FAM_HALS, 0, 0, NMFX_D_NONE, NMFX_D_NONE};      // (reads W, H and the Grams of nmfx_set_factors; derives nothing that outlives the call)
    if (!(tol >= 0.0 && tol < 1.0)) a.bad = std::string(who) + ": tol must be at least 0 and below 1";
    else if (max_sweeps < 1 || max_sweeps > 10000) a.bad = std::string(who) + ": max_sweeps must be between 1 and 10000";
    else if (!(lambda_h >= 0)) a.bad = std::string(who) + ": bad lambda";
    int rc = nmfx_enter(E, a); if (rc) return rc;
    E->run.in_place();
    if ((rc = nmfx_lazy_alloc(E, &S->foldin_sweeps, std::max<int64_t>(1, E->n)))) return rc;
    if (!S->masked) {
        if ((rc = nmfx_lazy_alloc(E, &S->hals_part, (int64_t)8 * E->ncu + 64))) return rc;
        if ((rc = nmfx_lazy_alloc(E, &S->side[1].slab64, std::max<int64_t>(1, S->side[1].npieces * E->kp)))) return rc;
    }
    if ((rc = objective_pass(E, NMFX_EU, E->W[0], &E->state->flag))) return rc;
    if ((rc = launch_objective(E, NMFX_EU, E->xf64, true, 0, SP_FOLDIN_NEVER, 0.0, 0.0))) return rc;
    const float tolf = (float)tol;
#define SP_FI(KP) (S->masked ? sp_mfoldin_solve<(KP) <= 64 ? (KP) : 64>(E, lambda_h, tolf, max_sweeps) : sp_foldin_solve<KP>(E, lambda_h, tolf, max_sweeps))
    switch (E->kp) { case 4: rc = SP_FI(4); break; case 8: rc = SP_FI(8); break; case 16: rc = SP_FI(16); break;
                     case 32: rc = SP_FI(32); break; case 64: rc = SP_FI(64); break; default: rc = SP_FI(128); break; }
#undef SP_FI
    if (rc) return rc;
    S->foldin_done = true;
    return NMFX_OK;
}

extern "C" int nmfx_hals_foldin_get_sweeps(nmfx_handle_t E, int32_t* out) {
    if (!E || !out) return NMFX_E_ARG;
    if (!E->sp || !E->sp->foldin_done) { E->err = "nmfx_hals_foldin_get_sweeps: no nmfx_hals_foldin_run since the factors were set"; return NMFX_E_STATE; }
    NMFX_HIP(hipSetDevice(E->device));
    NMFX_HIP(hipMemcpyAsync(out, E->sp->foldin_sweeps, (size_t)E->n * sizeof(int32_t), hipMemcpyDeviceToHost, E->stream));
    NMFX_HIP(hipStreamSynchronize(E->stream));
    return NMFX_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// MUR fold-in on a sparse handle (nmfx_sparse_foldin_run)
// ---------------------------------------------------------------------------------------------------------------------
// H for the handle's V against the W that was set, under the loss of sparse / masked MUR, W never touched.  With W fixed the
// columns of H are independent: a column takes the H half-step of sp_phase_kernel over and over, its iterate in the wave's
// registers (float4 per lane, the same bits in every group), until after step t
//     delta_t = max_j |h'_j - h_j| <= tol * max_j h'_j        (both in f32; delta_t = 0 counts)
// or max_iter.  What a step sums that does not depend on h is summed once, before the loop (FIXED):
//     Euclidean  a = Sum x_e w_e        masked KL  d = Sum w_e        (unmasked: G = W^T W and s = colsum W of nmfx_set_factors)
// and the loop sums the rest (STEP), q_e = <w_e, h> in f64 by the group butterfly:
//     KL  a = Sum x_e / (q_e + 1e-9) w_e      masked Euclidean  d = Sum (float) q_e w_e      IS  a = Sum x_e / q^2 w_e, d = Sum 1 / q w_e
// so on an unmasked handle a Euclidean step is k x k work against G (LDS for KP <= 128) and never touches the entries.  Lane
// layout, summation order and epilogue are those of sp_phase_kernel: a step of a column of at most SP_CHUNK entries is the H
// half-step bit for bit.  A column of more entries is one workgroup (sp_mur_foldin_long_kernel): the waves take its pieces
// wave, wave + SP_WAVES, ..., leave their [a | d] in LDS regions that are added in wave order, wave 0 runs the epilogue and the
// test and publishes h' and the decision through LDS.  No atomics; every loop bound and exit is wave- (block-) uniform.
template <int LOSS, bool MASKED> struct SpFi {
    static constexpr bool EU = LOSS == NMFX_EU, KL = LOSS == NMFX_KL, IS = LOSS == NMFX_IS;
    static constexpr bool FIXED_A = EU, FIXED_D = KL && MASKED;      // summed once
    static constexpr bool STEP_A = KL || IS, STEP_D = (EU && MASKED) || IS;   // summed per step
    static constexpr bool WALKS = STEP_A || STEP_D;                  // (false: unmasked Euclidean)
};

// One walk over the entries [beg, beg + len) of a column whose iterate is h4: FIXED, the sums formed once; else those of a step.
// acc / den are this lane's sums (before sp_sum_groups).
template <int KP, int LOSS, bool MASKED, bool FIXED>
__device__ __forceinline__ void sp_fi_walk(long long beg, int len, const int32_t* __restrict__ idx, const float* __restrict__ val,
                                           const float* __restrict__ W, float4 h4, float4& acc, float4& den, int lig, int grp)
{
    constexpr int G = KP / 4, NG = 64 / G;
    using F = SpFi<LOSS, MASKED>;
    const long long end = beg + len;
    for (long long e0 = beg + grp; e0 < end; e0 += 4 * NG) {
        int c[4]; float x[4]; bool ok[4]; float4 w[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const long long e = e0 + (long long)t * NG;
            ok[t] = e < end;
            c[t] = ok[t] ? idx[e] : 0;
            x[t] = ok[t] ? val[e] : 0.f;            // (a slot past the end gathers row 0 with weight 0)
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) w[t] = *reinterpret_cast<const float4*>(W + (int64_t)c[t] * KP + lig * 4);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            float qa = 0.f, qd = 0.f;
            if constexpr (FIXED) {
                qa = x[t]; qd = ok[t] ? 1.f : 0.f;
            } else {
                double wh = (double)h4.x * w[t].x + (double)h4.y * w[t].y + (double)h4.z * w[t].z + (double)h4.w * w[t].w;
#pragma unroll
                for (int off = 1; off < G; off <<= 1) wh += __shfl_xor(wh, off, 64);
                if constexpr (F::IS) {
                    const double iq = 1.0 / (wh + 1e-9);
                    qa = (float)((double)x[t] * iq * iq); qd = ok[t] ? (float)iq : 0.f;
                } else if constexpr (F::KL) {
                    qa = (float)((double)x[t] / (wh + 1e-9));
                } else {
                    qd = ok[t] ? (float)wh : 0.f;
                }
            }
            if constexpr (FIXED ? F::FIXED_A : F::STEP_A) {
                acc.x = fmaf(qa, w[t].x, acc.x); acc.y = fmaf(qa, w[t].y, acc.y);
                acc.z = fmaf(qa, w[t].z, acc.z); acc.w = fmaf(qa, w[t].w, acc.w);
            }
            if constexpr (FIXED ? F::FIXED_D : F::STEP_D) {
                den.x = fmaf(qd, w[t].x, den.x); den.y = fmaf(qd, w[t].y, den.y);
                den.z = fmaf(qd, w[t].z, den.z); den.w = fmaf(qd, w[t].w, den.w);
            }
        }
    }
}

// One step from h4 with the summed a4 / d4: the epilogue of the H half-step in registers, then the stop test.  delta and xmax
// over the components < k (the padding is 0 before and after) by one butterfly over the group's lanes, made uniform as
// sp_hals_sweeps<SOLVE> does.  Returns h'; *stop is wave-uniform.
template <int KP, int LOSS, bool MASKED>
__device__ __forceinline__ float4 sp_fi_step(float4 h4, float4 a4, float4 d4, const float* __restrict__ Gsrc, const float* __restrict__ S,
                                             float lam, int k, float tol, int lig, int grp, bool* stop)
{
    constexpr int G = KP / 4;
    using F = SpFi<LOSS, MASKED>;
    float4 o;
    if constexpr (MASKED) o = sp_epilogue_masked_value<F::KL, F::IS>(h4, a4, d4, lam, k, lig);
    else o = sp_epilogue_value<KP, F::KL>(h4, a4, Gsrc, S, lam, k, lig, grp);
    float delta = fmaxf(fmaxf(fabsf(o.x - h4.x), fabsf(o.y - h4.y)), fmaxf(fabsf(o.z - h4.z), fabsf(o.w - h4.w)));
    float xmax = fmaxf(fmaxf(o.x, o.y), fmaxf(o.z, o.w));
#pragma unroll
    for (int off = 1; off < G; off <<= 1) {
        delta = fmaxf(delta, __shfl_xor(delta, off, 64));
        xmax = fmaxf(xmax, __shfl_xor(xmax, off, 64));
    }
    delta = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(delta)));
    xmax = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(xmax)));
    *stop = delta <= tol * xmax;
    return o;
}

// Columns of at most SP_CHUNK entries (the units of side 1 with slot < 0): one wave per column.
//   W [m][KP]: gathered, never written; Ht [n][KP]: the iterate, read once and written once; Gf / S: W^T W and colsum W in f32
//   (unmasked handles); iters[col]: the steps the column took.
template <int KP, int LOSS, bool MASKED>
__global__ __launch_bounds__(64 * SP_WAVES) void sp_mur_foldin_kernel(
    const SpUnit* __restrict__ units, int64_t nunits, const int32_t* __restrict__ idx, const float* __restrict__ val,
    const float* __restrict__ W, float* __restrict__ Ht, const float* __restrict__ Gf, const float* __restrict__ S, float lam, int k,
    float tol, int max_iter, int32_t* __restrict__ iters, const int* flag)
{
    if (*flag) return;
    constexpr int G = KP / 4;
    using F = SpFi<LOSS, MASKED>;
    constexpr bool GLDS = F::EU && !MASKED && KP <= 128;
    __shared__ __attribute__((aligned(16))) float gs[GLDS ? KP * KP : 4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lig = lane % G, grp = lane / G;
    if constexpr (GLDS) {
        for (int i = tid * 4; i < KP * KP; i += 64 * SP_WAVES * 4)
            *reinterpret_cast<float4*>(gs + i) = *reinterpret_cast<const float4*>(Gf + i);
        __syncthreads();
    }
    const float* Gsrc = GLDS ? gs : Gf;
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int64_t u = (int64_t)blockIdx.x * SP_WAVES + wave; u < nunits; u += (int64_t)gridDim.x * SP_WAVES) {      // (no block barrier in here)
        const SpUnit U = units[u];
        if (U.slot >= 0) continue;                      // a piece of a long column: sp_mur_foldin_long_kernel (wave-uniform)
        float* row = Ht + (int64_t)U.row * KP;
        float4 h4 = *reinterpret_cast<const float4*>(row + lig * 4);
        float4 fa = zero, fd = zero;
        if constexpr (F::FIXED_A || F::FIXED_D) {
            sp_fi_walk<KP, LOSS, MASKED, true>(U.beg, U.len, idx, val, W, h4, fa, fd, lig, grp);
            if constexpr (F::FIXED_A) fa = sp_sum_groups<G>(fa);
            if constexpr (F::FIXED_D) fd = sp_sum_groups<G>(fd);
        }
        int t = 0;
        for (;;) {                                      // (bounded by max_iter; the exit is wave-uniform)
            float4 a4 = fa, d4 = fd;
            if constexpr (F::WALKS) {
                float4 sa = zero, sd = zero;
                sp_fi_walk<KP, LOSS, MASKED, false>(U.beg, U.len, idx, val, W, h4, sa, sd, lig, grp);
                if constexpr (F::STEP_A) a4 = sp_sum_groups<G>(sa);
                if constexpr (F::STEP_D) d4 = sp_sum_groups<G>(sd);
            }
            bool stop;
            h4 = sp_fi_step<KP, LOSS, MASKED>(h4, a4, d4, Gsrc, S, lam, k, tol, lig, grp, &stop);
            ++t;
            if (stop || t >= max_iter) break;
        }
        if (grp == 0) *reinterpret_cast<float4*>(row + lig * 4) = h4;
        if (lane == 0) iters[U.row] = t;
    }
}

// this wave's pieces of the long column L (wave, wave + SP_WAVES, ...) walked, and its [a | d] left in its LDS region
template <int KP, int LOSS, bool MASKED, bool FIXED>
__device__ __forceinline__ void sp_fi_deposit(const SpLong L, const SpUnit* __restrict__ units, const int32_t* __restrict__ idx,
                                              const float* __restrict__ val, const float* __restrict__ W, float4 h4, float* part,
                                              int wave, int lig, int grp)
{
    constexpr int G = KP / 4;
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f), d = a;
    for (int p = wave; p < L.npieces; p += SP_WAVES) {
        const SpUnit U = units[(int64_t)L.unit0 + p];
        sp_fi_walk<KP, LOSS, MASKED, FIXED>(U.beg, U.len, idx, val, W, h4, a, d, lig, grp);
    }
    a = sp_sum_groups<G>(a);
    d = sp_sum_groups<G>(d);
    if (grp == 0) {
        float* r = part + wave * (2 * KP) + lig * 4;
        *reinterpret_cast<float4*>(r) = a;
        *reinterpret_cast<float4*>(r + KP) = d;
    }
}

// the waves' regions added in wave order (every group reads the same words: the same bits)
template <int KP>
__device__ __forceinline__ void sp_fi_regions(const float* part, int lig, float4& a, float4& d) {
    a = make_float4(0.f, 0.f, 0.f, 0.f); d = a;
#pragma unroll
    for (int w = 0; w < SP_WAVES; ++w) {
        const float* r = part + w * (2 * KP) + lig * 4;
        a = sp_add4(a, *reinterpret_cast<const float4*>(r));
        d = sp_add4(d, *reinterpret_cast<const float4*>(r + KP));
    }
}

// Columns of more than SP_CHUNK entries: one workgroup per column (a blockIdx-strided loop: block-uniform, so every wave
// reaches every barrier).  Unmasked Euclidean: the pieces are walked once for a, then wave 0 steps alone against G.
template <int KP, int LOSS, bool MASKED>
__global__ __launch_bounds__(64 * SP_WAVES) void sp_mur_foldin_long_kernel(
    const SpLong* __restrict__ longs, int64_t nlong, const SpUnit* __restrict__ units, const int32_t* __restrict__ idx,
    const float* __restrict__ val, const float* __restrict__ W, float* __restrict__ Ht, const float* __restrict__ Gf,
    const float* __restrict__ S, float lam, int k, float tol, int max_iter, int32_t* __restrict__ iters, const int* flag)
{
    if (*flag) return;
    constexpr int G = KP / 4;
    using F = SpFi<LOSS, MASKED>;
    constexpr bool GLDS = F::EU && !MASKED && KP <= 128;
    __shared__ __attribute__((aligned(16))) float gs[GLDS ? KP * KP : 4];
    __shared__ __attribute__((aligned(16))) float part[SP_WAVES * 2 * KP];      // region w: wave w's [a | d]
    __shared__ __attribute__((aligned(16))) float hs[KP];                       // h' of the step
    __shared__ int go;                                                          // 1: another step
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lig = lane % G, grp = lane / G;
    if constexpr (GLDS) {
        for (int i = tid * 4; i < KP * KP; i += 64 * SP_WAVES * 4)
            *reinterpret_cast<float4*>(gs + i) = *reinterpret_cast<const float4*>(Gf + i);
        __syncthreads();
    }
    const float* Gsrc = GLDS ? gs : Gf;
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int64_t l = blockIdx.x; l < nlong; l += gridDim.x) {
        const SpLong L = longs[l];
        float* row = Ht + (int64_t)L.row * KP;
        float4 h4 = *reinterpret_cast<const float4*>(row + lig * 4);
        float4 fa = zero, fd = zero;                    // (wave 0's)
        if constexpr (F::FIXED_A || F::FIXED_D) {
            sp_fi_deposit<KP, LOSS, MASKED, true>(L, units, idx, val, W, h4, part, wave, lig, grp);
            __syncthreads();
            if (wave == 0) sp_fi_regions<KP>(part, lig, fa, fd);
            __syncthreads();                            // (the first step's deposits overwrite the regions)
        }
        int t = 0;
        if constexpr (!F::WALKS) {
            if (wave == 0) {
                for (;;) {
                    bool stop;
                    h4 = sp_fi_step<KP, LOSS, MASKED>(h4, fa, fd, Gsrc, S, lam, k, tol, lig, grp, &stop);
                    ++t;
                    if (stop || t >= max_iter) break;
                }
            }
        } else {
            for (;;) {                                  // (bounded by max_iter; every wave leaves on the same step)
                sp_fi_deposit<KP, LOSS, MASKED, false>(L, units, idx, val, W, h4, part, wave, lig, grp);
                __syncthreads();
                if (wave == 0) {
                    float4 a4, d4;
                    sp_fi_regions<KP>(part, lig, a4, d4);
                    if constexpr (!F::STEP_A) a4 = fa;
                    if constexpr (!F::STEP_D) d4 = fd;
                    bool stop;
                    const float4 o = sp_fi_step<KP, LOSS, MASKED>(h4, a4, d4, Gsrc, S, lam, k, tol, lig, grp, &stop);
                    if (grp == 0) *reinterpret_cast<float4*>(hs + lig * 4) = o;
                    if (lane == 0) go = (stop || t + 1 >= max_iter) ? 0 : 1;
                }
                __syncthreads();
                ++t;
                h4 = *reinterpret_cast<const float4*>(hs + lig * 4);
                if (!go) break;
            }
        }
        if (wave == 0) {
            if (grp == 0) *reinterpret_cast<float4*>(row + lig * 4) = h4;
            if (lane == 0) iters[L.row] = t;
        }
        __syncthreads();                                // (the next column's deposits and decision overwrite the LDS words)
    }
}

template <int KP, int LOSS, bool MASKED>
static int launch_mur_foldin(nmfx_engine* E, float lam, float tol, int max_iter) {
    nmfx_sparse* S = E->sp;
    SpSide& sd = S->side[1];
    const int* flag = &E->state->flag;
    const float* W = E->W[0];
    hipLaunchKernelGGL((sp_mur_foldin_kernel<KP, LOSS, MASKED>), dim3(sd.nblk), dim3(64 * SP_WAVES), 0, E->stream, (const SpUnit*)sd.units,
                       sd.nunits, (const int32_t*)sd.idx, (const float*)sd.val, W, S->Ht, (const float*)S->gf[0], (const float*)S->csf[0],
                       lam, E->k, tol, max_iter, S->mur_foldin_iters, flag);
    NMFX_HIP(hipGetLastError());
    if (sd.nlong) {
        const int nl = (int)std::min<int64_t>(4 * E->ncu, sd.nlong);
        hipLaunchKernelGGL((sp_mur_foldin_long_kernel<KP, LOSS, MASKED>), dim3(nl), dim3(64 * SP_WAVES), 0, E->stream,
                           (const SpLong*)sd.longs, sd.nlong, (const SpUnit*)sd.units, (const int32_t*)sd.idx, (const float*)sd.val, W,
                           S->Ht, (const float*)S->gf[0], (const float*)S->csf[0], lam, E->k, tol, max_iter, S->mur_foldin_iters, flag);
        NMFX_HIP(hipGetLastError());
    }
    return NMFX_OK;
}

// the solve, then on an unmasked handle the statistics of the new H (the objective reads them; they are current on return)
template <int KP>
static int sp_mur_foldin(nmfx_engine* E, int loss, float lam, float tol, int max_iter) {
    int rc;
    { ProfScope ps(E, "sp_mur_foldin");
      if (E->sp->masked)
          rc = loss == NMFX_IS ? launch_mur_foldin<KP, NMFX_IS, true>(E, lam, tol, max_iter)
             : loss == NMFX_KL ? launch_mur_foldin<KP, NMFX_KL, true>(E, lam, tol, max_iter)
                               : launch_mur_foldin<KP, NMFX_EU, true>(E, lam, tol, max_iter);
      else
          rc = loss == NMFX_KL ? launch_mur_foldin<KP, NMFX_KL, false>(E, lam, tol, max_iter)
                               : launch_mur_foldin<KP, NMFX_EU, false>(E, lam, tol, max_iter);
      if (rc) return rc; }
    if (!E->sp->masked) {
      ProfScope ps(E, "sp_stats");
      if ((rc = launch_stats<KP>(E, E->sp->Ht, E->n, 1, &E->state->flag))) return rc; }
    return NMFX_OK;
}

extern "C" int nmfx_sparse_foldin_run(nmfx_handle_t E, int distance, double lambda_h, double tol, int max_iter) {
    const std::string who = "nmfx_sparse_foldin_run";
    if (!E) return NMFX_E_ARG;
    if (!E->sp) { E->err = who + ": needs a sparse handle (nmfx_create_csr), masked or not; a dense handle runs nmfx_foldin_run"; return NMFX_E_ARG; }
    nmfx_sparse* S = E->sp;
    nmfx_entry a = {NMFX_FAM_MUR, 0, 0, NMFX_D_NONE, NMFX_D_NONE};      // (derives nothing from (W, H) that outlives the call)
    if (distance == NMFX_IS && !S->masked)
        a.bad = who + ": the Itakura-Saito divergence (IS) is infinite at the zeros of an unmasked sparse V: make the handle masked (nmfx_set_masked)";
    else if (distance != NMFX_EU && distance != NMFX_KL && distance != NMFX_IS)
        a.bad = who + ": the distance must be NMFX_EU, NMFX_KL or (masked handles) NMFX_IS";
    else if (!(tol >= 0.0 && tol < 1.0)) a.bad = who + ": tol must be at least 0 and below 1";
    else if (max_iter < 1 || max_iter > 10000) a.bad = who + ": max_iter must be between 1 and 10000";
    else if (!(lambda_h >= 0)) a.bad = who + ": bad lambda";
    else if (E->run.started && !S->mur_foldin_done) {   // (MUR has ping-ponged W since: W[0] need not be the current one)
        a.bad = who + ": nmfx_mur_run has iterated on this handle since nmfx_set_factors: set the factors again first";
        a.bad_rc = NMFX_E_STATE;
    }
    int rc = nmfx_enter(E, a); if (rc) return rc;
    E->run.mur_loss(distance);
    E->run.in_place();                                 // (W[0], never written; H^T in place)
    if ((rc = nmfx_lazy_alloc(E, &S->mur_foldin_iters, std::max<int64_t>(1, E->n)))) return rc;
    const int* flag = &E->state->flag;
    if ((rc = objective_pass(E, distance, E->W[0], flag))) return rc;
    if ((rc = launch_objective(E, distance, E->xf64, true, 0, SP_FOLDIN_NEVER, 0.0, 0.0))) return rc;
#define SP_MFI(KP) sp_mur_foldin<KP>(E, distance, (float)lambda_h, (float)tol, max_iter)
    switch (E->kp) { case 4: rc = SP_MFI(4); break; case 8: rc = SP_MFI(8); break; case 16: rc = SP_MFI(16); break;
                     case 32: rc = SP_MFI(32); break; case 64: rc = SP_MFI(64); break; case 128: rc = SP_MFI(128); break;
                     default: rc = SP_MFI(256); break; }
#undef SP_MFI
    if (rc) return rc;
    if ((rc = objective_pass(E, distance, E->W[0], flag))) return rc;
    if ((rc = launch_objective(E, distance, E->xf64, true, 1, SP_FOLDIN_NEVER, 0.0, 0.0))) return rc;
    S->mur_foldin_done = true;
    return NMFX_OK;
}

extern "C" int nmfx_sparse_foldin_get_iters(nmfx_handle_t E, int32_t* out) {
    if (!E || !out) return NMFX_E_ARG;
    if (!E->sp || !E->sp->mur_foldin_done) { E->err = "nmfx_sparse_foldin_get_iters: no nmfx_sparse_foldin_run since the factors were set"; return NMFX_E_STATE; }
    NMFX_HIP(hipSetDevice(E->device));
    NMFX_HIP(hipMemcpyAsync(out, E->sp->mur_foldin_iters, (size_t)E->n * sizeof(int32_t), hipMemcpyDeviceToHost, E->stream));
    NMFX_HIP(hipStreamSynchronize(E->stream));
    return NMFX_OK;
}

int nmfx_preload_sparse() { hipFuncAttributes a; return hipFuncGetAttributes(&a, reinterpret_cast<const void*>(sp_stats_reduce_kernel)) == hipSuccess ? 0 : -1; }
