// MUR with per-entry weights Omega >= 0 (nmfx_upload_weights), dense V, k <= 128, exact f32.  T = W H, W' = the new W.
//
//   Euclidean  W <- W o ((Om o V) H^T) / ((Om o T) H^T + lam_w W + 1e-9)                      objective  1/2 Sum om (v - T)^2
//   KL         A = W o ((Om o V / (T + 1e-9)) H^T),  B = Om H^T,
//              W <- 2 A / (B + sqrt(B^2 + 4 lam_w A)),  0 where B = 0                         Sum om [v log(v / T) - v + T]
//   IS         q = T + 1e-9,  W <- W o sqrt( ((Om o V / q^2) H^T) / ((Om / q) H^T + lam_w) ),  0 where the denominator is 0
//                                                                                             Sum om [v / q - log(v / q) - 1]
//   H likewise with W' and lam_h.  A cell with om = 0 is unknown: V is not part of any sum there.
//
// The kernels are those of kernels_is.hip with a second V-sized stream and a loss parameter.  Both phases are ONE template
// with the roles of the factors swapped (wt_phase_kernel).  Per 16-wide stage of the contracted dimension a wave loads its
// V slice and the Omega slice in the same register layout, forms the tile of T with the f32 MFMA in that layout, derives
// the loss's two per-entry quantities in registers
//     Euclidean  num = om v,              den = om T
//     KL         num = om v / (T + 1e-9), den = om
//     IS         num = om v / q^2,        den = om / q
// and feeds each into a second MFMA product: two accumulators (numerator, denominator) per output tile.  The W phase also
// sums the objective terms of the pair it starts from (f32 per stage, f64 across stages).  Slabs [num | den] of the split
// contracted dimension are summed in slab order by the update kernels: no atomics, two runs are bit-identical.
//
// Zero weight and zero padding.  Padded cells of V and Omega are 0.  Wherever om = 0 -- padding or an unknown cell -- num,
// den and the objective term are SELECTED to 0 (om > 0 ? ... : 0), never multiplied to 0: what the other branch holds
// there (1 / 1e-9 from a zero T, 0 / 0, the logarithm of 0, whatever bits V has) is discarded, so no 0 * 1e9 or 0 * inf
// product is ever formed and every loss gives exact zeros.  A padded factor component multiplies finite num / den by its
// zero entries (exact 0) and the update kernels write 0 there without reading the sums.  A padded row / column of the kept
// index, like a real one without any weight, receives num = den = 0 and its closed form gives 0: Euclidean 0 / (lam w +
// 1e-9), KL B = 0 -> 0, IS den + lam = 0 -> 0 and w sqrt(0 / lam) = 0 otherwise.
#include "nmfx_internal.h"
#include "kernels_small.h"

#define MFMA(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)

// --------------------------------------------------------------------------
// One phase.  "Kept" index u: a column of V (H phase) / a row of V (W phase); "contracted" index s: the other one.
//   F  = the factor along s:  F[s][c] = W[s][c] (H phase) / H[c][s] (W phase)
//   P  = the panel of the factor along u, in LDS: P[c][i] = H[c][u0 + i] (H phase) / W[u0 + i][c] (W phase)
// Block = 16 NE kept indices x the contracted range of split blockIdx.y, its 16-wide stages dealt to the 4 waves.
// Stage:
//   T tile e  = F(16 x KP) . P(KP x 16)              -> lane (x, q) reg r = (W H) at (s0 + 4q + r, u0 + 16e + x)
//   num, den per entry by LOSS (V and Omega loaded in that same layout)
//   nacc[j][e] += F(4 stage rows, tile j)^T . num(4 stage rows, tile e),  dacc likewise with den     for the 4 groups r
// Output slab of split sr: [num | den], each [KP][np] (H phase) / [mp][KP] (W phase).
// --------------------------------------------------------------------------
template <int LOSS, int KP, int NE, bool WPH, bool UPD, bool OBJ>
__global__ __launch_bounds__(256) void wt_phase_kernel(
    const float* __restrict__ V, const float* __restrict__ Om, int64_t ldv, const float* __restrict__ W,
    const float* __restrict__ H, float* __restrict__ part, double* __restrict__ objpart, int64_t np, int64_t mp,
    const int* __restrict__ flag)
{
    if (*flag) return;
    constexpr int JT = KP / 16;
    constexpr int LDP = 16 * NE + 4;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, x = lane & 15, q = lane >> 4;
    const int SR = gridDim.y, sr = blockIdx.y;
    const int64_t k0 = (int64_t)blockIdx.x * 16 * NE;
    const int64_t n16 = (WPH ? np : mp) / 16;
    const int64_t u0 = n16 * sr / SR, u1 = n16 * (sr + 1) / SR;
    const int64_t t0 = u0 + (u1 - u0) * wave / 4, t1 = u0 + (u1 - u0) * (wave + 1) / 4;

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
        float fa[JT][4], fb[4][UPD ? JT : 1], vv[NE][4], om[NE][4];
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
                const float4 o = *reinterpret_cast<const float4*>(Om + at);
                vv[e][0] = v.x; vv[e][1] = v.y; vv[e][2] = v.z; vv[e][3] = v.w;
                om[e][0] = o.x; om[e][1] = o.y; om[e][2] = o.z; om[e][3] = o.w;
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
                    om[e][r] = Om[at];
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
        // per entry: vv <- num, pe <- den, both selected to 0 where the weight is 0 (header)
        float part_obj = 0.f;
#pragma unroll
        for (int e = 0; e < NE; ++e)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float w = om[e][r], v = vv[e][r], T = pe[e][r];
                const bool live = w > 0.f;
                float nu, de, term = 0.f;
                if (LOSS == NMFX_EU) {
                    const float d = v - T;
                    term = w * (d * d);
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
                if (OBJ) part_obj += live ? term : 0.f;
                vv[e][r] = live ? nu : 0.f;
                pe[e][r] = live ? de : 0.f;
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
        if (LOSS == NMFX_EU) osum *= 0.5;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) osum += __shfl_down(osum, off, 64);
        double* ored = reinterpret_cast<double*>(lds);
        if (lane == 0) ored[wave] = osum;
        __syncthreads();
        if (tid == 0) objpart[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = ((ored[0] + ored[1]) + ored[2]) + ored[3];
    }
}

// The three closed forms on f = the old factor entry, a / d = the summed numerator / denominator
__device__ __forceinline__ float wt_closed_form(int loss, float f, float a, float d, float lam) {
    if (loss == NMFX_EU) return (f * a) / ((d + lam * f) + 1e-9f);
    if (loss == NMFX_KL) {
        const float A = f * a;
        return d > 0.f ? (2.f * A) / (d + sqrtf(d * d + (4.f * lam) * A)) : 0.f;
    }
    d += lam;
    return d > 0.f ? f * sqrtf(a / d) : 0.f;
}

// W_new from the slabs' numerators / denominators, summed in slab order
__global__ __launch_bounds__(256) void wt_w_update_kernel(
    const float* __restrict__ part, int splits, int64_t count, int kp, int k, int loss, const float* __restrict__ Wold, float lam,
    float* __restrict__ Wnew, const int* __restrict__ flag)
{
    if (*flag) return;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    if ((int)(i % kp) >= k) { Wnew[i] = 0.f; return; }       // padded factors stay zero
    float a = part[i], d = part[count + i];
    for (int p = 1; p < splits; ++p) { a += part[(int64_t)(2 * p) * count + i]; d += part[(int64_t)(2 * p + 1) * count + i]; }
    Wnew[i] = wt_closed_form(loss, Wold[i], a, d, lam);
}

// H_new after the objective bookkeeping / convergence test (same protocol as MUR-KL and MUR-IS)
__global__ __launch_bounds__(256) void wt_h_update_kernel(
    const float* __restrict__ part, int splits, const double* __restrict__ xf64, float* __restrict__ H, int64_t np, int kp,
    int k, int loss, float lam, long long j, long long min_iter, double tol1, double tol2, DevState* __restrict__ st,
    double* __restrict__ obj_hist)
{
    if (st->flag) return;
    const int rule = nmfx_record_objective(st, obj_hist, xf64[0], j, min_iter, tol1, tol2,
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
    float4 o;
    o.x = wt_closed_form(loss, h.x, a.x, d.x, lam);
    o.y = wt_closed_form(loss, h.y, a.y, d.y, lam);
    o.z = wt_closed_form(loss, h.z, a.z, d.z, lam);
    o.w = wt_closed_form(loss, h.w, a.w, d.w, lam);
    *reinterpret_cast<float4*>(H + i) = o;
}

// --------------------------------------------------------------------------
// Splits of the contracted dimension: enough blocks for two per CU, at least 8 stages (2 per wave) each
static int wt_splits(const nmfx_engine* E, int64_t blocks_x, int64_t stages) {
    const int64_t want = (2 * (int64_t)E->ncu + blocks_x - 1) / blocks_x;
    return (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(want, 16), stages / 8));
}
static int wt_ne(int kp) { return kp == 128 ? 2 : 4; }
static int wt_wsplits(const nmfx_engine* E) { return wt_splits(E, E->mp / (16 * wt_ne(E->kp)), E->np / 16); }
static int wt_hsplits(const nmfx_engine* E) { return wt_splits(E, E->np / (16 * wt_ne(E->kp)), E->mp / 16); }

// slabs of both phases share one buffer (the one MUR-IS uses: the two never run at the same time on a handle's stream)
static int wt_ensure(nmfx_engine* E) {
    const int64_t need = 2 * std::max<int64_t>((int64_t)wt_wsplits(E) * E->mp * E->kp, (int64_t)wt_hsplits(E) * E->kp * E->np);
    if (E->is_part && E->is_part_cap >= need) return NMFX_OK;
    if (E->is_part) { NMFX_HIP(hipStreamSynchronize(E->stream)); NMFX_HIP(hipFree(E->is_part)); E->is_part = nullptr; E->is_part_cap = 0; }
    NMFX_HIP(hipMalloc(reinterpret_cast<void**>(&E->is_part), (size_t)need * sizeof(float)));
    E->is_part_cap = need;
    return NMFX_OK;
}

template <int LOSS, int KP, int NE>
static int launch_wt_phase(nmfx_engine* E, bool wph, bool upd, const float* W) {
    const int splits = wph ? wt_wsplits(E) : wt_hsplits(E);
    dim3 grid((unsigned)((wph ? E->mp : E->np) / (16 * NE)), (unsigned)splits), block(256);
    const size_t panel = (size_t)KP * (16 * NE + 4) * sizeof(float);
    const size_t red = (size_t)2 * (KP / 16) * NE * 64 * sizeof(f32x4);
    const size_t shm = std::max(panel, red);
    { int rc_ = nmfx_need_v(E); if (rc_) return rc_; }
    if (wph) {
        E->obj_count = (int64_t)grid.x * grid.y;
        if (E->obj_count > E->obj_part_cap) { E->err = "weighted MUR: objective partials exceed their buffer"; return NMFX_E_ARG; }
    }
#define NMFX_WTLAUNCH(WP, UP, OB) \
    hipLaunchKernelGGL((wt_phase_kernel<LOSS, KP, NE, WP, UP, OB>), grid, block, shm, E->stream, E->V, E->Om, E->np, W, E->H, \
                       E->is_part, E->obj_part, E->np, E->mp, &E->state->flag)
    if (wph) { if (upd) NMFX_WTLAUNCH(true, true, true); else NMFX_WTLAUNCH(true, false, true); }
    else NMFX_WTLAUNCH(false, true, false);
#undef NMFX_WTLAUNCH
    NMFX_HIP(hipGetLastError());
    return NMFX_OK;
}

template <int LOSS>
static int wt_phase_kp(nmfx_engine* E, bool wph, bool upd, const float* W) {
    switch (E->kp) {
        case 16: return launch_wt_phase<LOSS, 16, 4>(E, wph, upd, W);
        case 32: return launch_wt_phase<LOSS, 32, 4>(E, wph, upd, W);
        case 64: return launch_wt_phase<LOSS, 64, 4>(E, wph, upd, W);
        case 128: return launch_wt_phase<LOSS, 128, 2>(E, wph, upd, W);
    }
    E->err = "weighted MUR: unsupported padded rank";
    return NMFX_E_ARG;
}

static int wt_phase(nmfx_engine* E, int distance, bool wph, bool upd, const float* W) {
    if (!E->Om) { E->err = "weighted MUR: no weights uploaded"; return NMFX_E_STATE; }
    switch (distance) {
        case NMFX_EU: return wt_phase_kp<NMFX_EU>(E, wph, upd, W);
        case NMFX_KL: return wt_phase_kp<NMFX_KL>(E, wph, upd, W);
        case NMFX_IS: return wt_phase_kp<NMFX_IS>(E, wph, upd, W);
    }
    E->err = "Unknown distance type.";
    return NMFX_E_ARG;
}

int nmfx_mur_wt_phase_a(nmfx_engine* E, int distance, double lambda_w, int64_t j) {
    const float* Wold = E->W[j & 1];
    float* Wnew = E->W[(j + 1) & 1];
    int rc;
    if ((rc = wt_ensure(E))) return rc;
    { ProfScope ps(E, "wt_wphase");
      if ((rc = wt_phase(E, distance, true, true, Wold))) return rc; }
    { ProfScope ps(E, "w_update");
      const int64_t count = E->mp * E->kp;
      hipLaunchKernelGGL(wt_w_update_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, E->stream, E->is_part,
                         wt_wsplits(E), count, E->kp, E->k, distance, Wold, (float)lambda_w, Wnew, &E->state->flag);
      NMFX_HIP(hipGetLastError()); }
    { ProfScope ps(E, "wt_hphase");
      if ((rc = wt_phase(E, distance, false, true, Wnew))) return rc; }
    return nmfx_launch_obj_reduce(E, E->obj_count);
}

int nmfx_mur_wt_phase_b(nmfx_engine* E, int distance, double lambda_h, int64_t min_iter, double tol1, double tol2, int64_t j) {
    ProfScope ps(E, "h_update");
    const int64_t n4 = ((int64_t)E->kp * E->np) / 4;
    hipLaunchKernelGGL(wt_h_update_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, E->stream, E->is_part,
                       wt_hsplits(E), E->xf64, E->H, E->np, E->kp, E->k, distance, (float)lambda_h, (long long)j,
                       (long long)min_iter, tol1, tol2, E->state, E->obj_hist);
    NMFX_HIP(hipGetLastError());
    return NMFX_OK;
}

int nmfx_mur_wt_finish_a(nmfx_engine* E, int distance, int64_t j) {
    int rc;
    { ProfScope ps(E, "objective");
      if ((rc = wt_phase(E, distance, true, false, E->W[j & 1]))) return rc; }
    return nmfx_launch_obj_reduce(E, E->obj_count);
}

// (nmfx_create: forces this translation unit's code object onto the device under the library's start-up lock)
int nmfx_preload_weighted() { hipFuncAttributes a; return hipFuncGetAttributes(&a, reinterpret_cast<const void*>(wt_w_update_kernel)) == hipSuccess ? 0 : -1; }
