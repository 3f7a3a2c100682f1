// HALS: hierarchical alternating least squares (Cichocki & Phan 2009; scikit-learn's solver = 'cd').
//
// A half-step works on the per-problem data of an ANLS half-step (kernels_anls.hip): the shared Gram matrix
// G = F^T F + 2 lambda I and one right-hand side r = F^T b per row of W / column of H.  Where ANLS solves every problem
// exactly, HALS makes `sweeps` projected Gauss-Seidel sweeps over the k components from the current solution x >= 0:
//     for j = 0 .. k-1:  if G_jj > 0:  x_j <- max(0, x_j + (r_j - sum_l G_jl x_l) / G_jj)      (x_0 .. x_{j-1} already new)
// A component with G_jj = 0 (dead, at lambda = 0) keeps its value.  The clamp is an exact zero.
//
// One wavefront owns one problem, variable i on lane i (at kp = 128: i and i + 64).  The wave keeps the residual
// g = r - G x in registers: one mat-vec per problem, and step j is
//     delta = max(-x_j, g_j / G_jj) on lane j, broadcast (v_readlane);  x_j += delta;  g_i -= delta G_ij on every lane
// (the lane keeps -x_j, the lower bound of its step, instead of x_j)
// so that further sweeps need no new mat-vec.  G is symmetric, column j is row j: it is read from a copy of G in LDS that the
// block stages once (2 lambda already on its diagonal), consecutive lanes on consecutive addresses, and the blocks loop over
// the problems.  Every loop bound is wave-uniform (k, sweeps, the problem index); there are no atomics, and the order of every
// sum is fixed: two runs give the same bits.  Rows, columns and lanes at or beyond k are never read into a sum; the padded
// variables are written back as exact zeros.
#include "nmfx_internal.h"

#define NMFX_HALS_WAVES 8                 // problems a block works on at a time
#define NMFX_HALS_BLOCKS_PER_CU 2         // one round of the grid (kp = 128: the 64 KiB copy of G lets a CU hold two blocks)

// this lane's entries of row `j` of the LDS copy of G
template <int KP, int NV>
__device__ __forceinline__ void hals_row(const float* gs, int j, const int (&at)[NV], float (&out)[NV]) {
#pragma unroll
    for (int t = 0; t < NV; ++t) out[t] = gs[j * KP + at[t]];
}

template <int KP>
__global__ __launch_bounds__(64 * NMFX_HALS_WAVES) void hals_sweep_kernel(
    const float* __restrict__ G, float diag_add, const float* __restrict__ R, float* __restrict__ X,
    int64_t sj, int64_t sc, int64_t nprob, int k, int sweeps, const DevState* __restrict__ st)
{
    if (st->flag) return;                               // (the stop rule has fired: the iterate stays)
    constexpr int NV = KP <= 64 ? 1 : KP / 64;          // variables per lane
    constexpr int NW = NMFX_HALS_WAVES;
    extern __shared__ __attribute__((aligned(16))) float hals_g[];      // G + diag_add I, [KP][KP]
    for (int i4 = threadIdx.x; i4 < KP * KP / 4; i4 += 64 * NW) {
        float4 v = *reinterpret_cast<const float4*>(G + 4 * (int64_t)i4);
        const int row = (4 * i4) / KP, col = (4 * i4) % KP;
        v.x += (col == row) ? diag_add : 0.f; v.y += (col + 1 == row) ? diag_add : 0.f;
        v.z += (col + 2 == row) ? diag_add : 0.f; v.w += (col + 3 == row) ? diag_add : 0.f;
        *reinterpret_cast<float4*>(hals_g + 4 * i4) = v;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int at[NV]; bool valid[NV], live[NV]; float inv[NV];
#pragma unroll
    for (int t = 0; t < NV; ++t) {
        const int idx = lane + 64 * t;
        valid[t] = idx < k;
        at[t] = idx < KP ? idx : KP - 1;                // (lanes beyond KP at kp = 16 / 32: any address inside the row; their values are unused)
        const float gd = hals_g[at[t] * KP + at[t]];
        live[t] = valid[t] && gd > 0.f;
        inv[t] = live[t] ? 1.f / gd : 0.f;
    }
    for (int64_t c = (int64_t)blockIdx.x * NW + wave; c < nprob; c += (int64_t)gridDim.x * NW) {      // (wave-uniform)
        float x[NV], g[NV], nx[NV];
#pragma unroll
        for (int t = 0; t < NV; ++t) {
            const int64_t off = (int64_t)at[t] * sj + c * sc;
            x[t] = valid[t] ? X[off] : 0.f;
            g[t] = valid[t] ? R[off] : 0.f;
            nx[t] = live[t] ? -x[t] : 0.f;              // the lower bound of a step, max(-x_j, .); 0 with inv = 0 where G_jj = 0: a step of 0
        }
        // g = r - G x: column l of G (= row l) against x_l, broadcast from its lane.  Both loops go four rows at a time, so that
        // the four LDS reads are in flight together (written out: v_readlane is convergent and the trip count is not a constant).
        auto matvec = [&](int t2, int l, const float (&col)[NV]) {
            const float xl = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x[t2]), l));
#pragma unroll
            for (int t = 0; t < NV; ++t) g[t] = fmaf(-col[t], xl, g[t]);
        };
        // step j: every lane forms its own candidate from its current g; lane j's is the step of variable 64 t2 + j
        auto step = [&](int t2, int j, const float (&col)[NV]) {
            const float cand = fmaxf(nx[t2], g[t2] * inv[t2]);
            const float d = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(cand), j));
            nx[t2] = (lane == j) ? nx[t2] - d : nx[t2];          // (d = -x_j: an exact zero)
#pragma unroll
            for (int t = 0; t < NV; ++t) g[t] = fmaf(-col[t], d, g[t]);
        };
#pragma unroll
        for (int t2 = 0; t2 < NV; ++t2) {
            const int lim = k - 64 * t2 < 64 ? k - 64 * t2 : 64;
            int l = 0;
            for (; l + 4 <= lim; l += 4) {
                float c0[NV], c1[NV], c2[NV], c3[NV];
                hals_row<KP, NV>(hals_g, 64 * t2 + l, at, c0); hals_row<KP, NV>(hals_g, 64 * t2 + l + 1, at, c1);
                hals_row<KP, NV>(hals_g, 64 * t2 + l + 2, at, c2); hals_row<KP, NV>(hals_g, 64 * t2 + l + 3, at, c3);
                matvec(t2, l, c0); matvec(t2, l + 1, c1); matvec(t2, l + 2, c2); matvec(t2, l + 3, c3);
            }
            for (; l < lim; ++l) {
                float c0[NV];
                hals_row<KP, NV>(hals_g, 64 * t2 + l, at, c0);
                matvec(t2, l, c0);
            }
        }
        for (int s = 0; s < sweeps; ++s) {
#pragma unroll
            for (int t2 = 0; t2 < NV; ++t2) {
                const int lim = k - 64 * t2 < 64 ? k - 64 * t2 : 64;
                int j = 0;
                for (; j + 4 <= lim; j += 4) {
                    float c0[NV], c1[NV], c2[NV], c3[NV];
                    hals_row<KP, NV>(hals_g, 64 * t2 + j, at, c0); hals_row<KP, NV>(hals_g, 64 * t2 + j + 1, at, c1);
                    hals_row<KP, NV>(hals_g, 64 * t2 + j + 2, at, c2); hals_row<KP, NV>(hals_g, 64 * t2 + j + 3, at, c3);
                    step(t2, j, c0); step(t2, j + 1, c1); step(t2, j + 2, c2); step(t2, j + 3, c3);
                }
                for (; j < lim; ++j) {
                    float c0[NV];
                    hals_row<KP, NV>(hals_g, 64 * t2 + j, at, c0);
                    step(t2, j, c0);
                }
            }
        }
#pragma unroll
        for (int t = 0; t < NV; ++t)
            if (lane + 64 * t < KP) X[(int64_t)at[t] * sj + c * sc] = live[t] ? 0.f - nx[t] : x[t];      // (0 - 0: +0; invalid lanes hold x = 0)
    }
}

template <int KP>
static int launch_hals_sweep(nmfx_engine* E, const float* G, float diag_add, const float* R, float* X, int64_t sj, int64_t sc,
                             int64_t nprob, int sweeps) {
    int rc;
    const size_t shm = (size_t)KP * KP * sizeof(float);
    auto kern = hals_sweep_kernel<KP>;
    if ((rc = nmfx_allow_lds(E, reinterpret_cast<const void*>(kern), (int)shm))) return rc;
    const int64_t blocks_needed = (nprob + NMFX_HALS_WAVES - 1) / NMFX_HALS_WAVES;
    const int64_t round = (int64_t)E->ncu * NMFX_HALS_BLOCKS_PER_CU;
    const unsigned grid = (unsigned)(blocks_needed < round ? blocks_needed : round);
    hipLaunchKernelGGL(kern, dim3(grid), dim3(64 * NMFX_HALS_WAVES), shm, E->stream, G, diag_add, R, X, sj, sc, nprob, E->k,
                       sweeps, E->state);
    NMFX_HIP(hipGetLastError());
    return NMFX_OK;
}

// Same arguments and stride conventions as the NNLS launcher of kernels_anls.hip (W: sj = 1, sc = kp; H: sj = np, sc = 1).
int nmfx_hals_sweep(nmfx_engine* E, const float* G, float diag_add, const float* R, float* X, int64_t sj, int64_t sc,
                    int64_t nprob, int sweeps) {
    ProfScope ps(E, "hals_sweep");
    if (nprob <= 0) return NMFX_OK;
    switch (E->kp) {
        case 16: return launch_hals_sweep<16>(E, G, diag_add, R, X, sj, sc, nprob, sweeps);
        case 32: return launch_hals_sweep<32>(E, G, diag_add, R, X, sj, sc, nprob, sweeps);
        case 64: return launch_hals_sweep<64>(E, G, diag_add, R, X, sj, sc, nprob, sweeps);
        case 128: return launch_hals_sweep<128>(E, G, diag_add, R, X, sj, sc, nprob, sweeps);
    }
    E->err = nmfx_small_k_text("hals_sweep");
    return NMFX_E_ARG;
}

// (nmfx_create: forces this translation unit's code object onto the device under the library's start-up lock)
int nmfx_preload_hals() { hipFuncAttributes a; return hipFuncGetAttributes(&a, reinterpret_cast<const void*>(hals_sweep_kernel<128>)) == hipSuccess ? 0 : -1; }
