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

// STACK (nmfx_hals_stack_*): the k components are P problems side by side.  While G is staged, an entry whose row and column
// belong to different problems, or to none, is stored as zero and the diagonal gets its own problem's 2 lambda_p (sk->diag[side]):
// the sweep over the stacked components is then P independent sweeps -- a masked term is fmaf(-0 d, ., g) = g, bit for bit.  A
// component of a stopped problem, or of none, is not live: its steps are exact zeros and its x is written back as it was read.
// The stop state is read once per launch, before the loop over the problems.
template <int KP, bool STACK = false>
__global__ __launch_bounds__(64 * NMFX_HALS_WAVES) void hals_sweep_kernel(
    const float* __restrict__ G, float diag_add, const float* __restrict__ R, float* __restrict__ X,
    int64_t sj, int64_t sc, int64_t nprob, int k, int sweeps, const DevState* __restrict__ st,
    const HalsStackDev* __restrict__ sk = nullptr, int side = 0)
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
        if constexpr (STACK) {
            v = *reinterpret_cast<const float4*>(G + 4 * (int64_t)i4);
            const unsigned pr = sk->c2p[row];
            const unsigned pc4 = *reinterpret_cast<const unsigned*>(sk->c2p + col);       // (col is a multiple of 4)
            const float dg = sk->diag[side][row];                                          // (0 for a component of no problem)
            const bool own = pr != NMFX_STACK_NONE;
            v.x = (own && (pc4 & 255u) == pr) ? v.x : 0.f;          v.y = (own && ((pc4 >> 8) & 255u) == pr) ? v.y : 0.f;
            v.z = (own && ((pc4 >> 16) & 255u) == pr) ? v.z : 0.f;  v.w = (own && (pc4 >> 24) == pr) ? v.w : 0.f;
            v.x += (col == row) ? dg : 0.f; v.y += (col + 1 == row) ? dg : 0.f;
            v.z += (col + 2 == row) ? dg : 0.f; v.w += (col + 3 == row) ? dg : 0.f;
        }
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
        if constexpr (STACK) {
            const unsigned p = sk->c2p[at[t]];
            live[t] = live[t] && p != NMFX_STACK_NONE && sk->pflag[p < NMFX_STACK_MAX ? p : 0] == 0;
        }
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

template <int KP, bool STACK>
static int launch_hals_sweep(nmfx_engine* E, const float* G, float diag_add, const float* R, float* X, int64_t sj, int64_t sc,
                             int64_t nprob, int sweeps, int side) {
    int rc;
    const size_t shm = (size_t)KP * KP * sizeof(float);
    auto kern = hals_sweep_kernel<KP, STACK>;
    if ((rc = nmfx_allow_lds(E, reinterpret_cast<const void*>(kern), (int)shm))) return rc;
    const int64_t blocks_needed = (nprob + NMFX_HALS_WAVES - 1) / NMFX_HALS_WAVES;
    const int64_t round = (int64_t)E->ncu * NMFX_HALS_BLOCKS_PER_CU;
    const unsigned grid = (unsigned)(blocks_needed < round ? blocks_needed : round);
    hipLaunchKernelGGL(kern, dim3(grid), dim3(64 * NMFX_HALS_WAVES), shm, E->stream, G, diag_add, R, X, sj, sc, nprob, E->k,
                       sweeps, E->state, STACK ? E->stack_dev : nullptr, side);
    NMFX_HIP(hipGetLastError());
    return NMFX_OK;
}

// the one kp dispatch of the sweep, plain and stacked
template <bool STACK>
static int hals_sweep_kp(nmfx_engine* E, const float* G, float diag_add, const float* R, float* X, int64_t sj, int64_t sc,
                         int64_t nprob, int sweeps, int side) {
    switch (E->kp) {
        case 16: return launch_hals_sweep<16, STACK>(E, G, diag_add, R, X, sj, sc, nprob, sweeps, side);
        case 32: return launch_hals_sweep<32, STACK>(E, G, diag_add, R, X, sj, sc, nprob, sweeps, side);
        case 64: return launch_hals_sweep<64, STACK>(E, G, diag_add, R, X, sj, sc, nprob, sweeps, side);
        case 128: return launch_hals_sweep<128, STACK>(E, G, diag_add, R, X, sj, sc, nprob, sweeps, side);
    }
    E->err = nmfx_small_k_text(STACK ? "hals_stack_sweep" : "hals_sweep");
    return NMFX_E_ARG;
}

// Same arguments and stride conventions as the NNLS launcher of kernels_anls.hip (W: sj = 1, sc = kp; H: sj = np, sc = 1).
// stack_side >= 0: the stacked form (nmfx_internal.h); its diagonal comes from the stack's own lambdas, not from diag_add.
int nmfx_hals_sweep(nmfx_engine* E, const float* G, float diag_add, const float* R, float* X, int64_t sj, int64_t sc,
                    int64_t nprob, int sweeps, int stack_side) {
    ProfScope ps(E, "hals_sweep");
    ProfScope side(E, sc == 1 ? "hals_sweep_h" : "hals_sweep_w");          // (the same launch under its side's name: tools/hals_transform_perf.py --dense)
    if (nprob <= 0) return NMFX_OK;
    return stack_side < 0 ? hals_sweep_kp<false>(E, G, diag_add, R, X, sj, sc, nprob, sweeps, 0)
                          : hals_sweep_kp<true>(E, G, 0.f, R, X, sj, sc, nprob, sweeps, stack_side);
}

// ---- beyond 128 components: G streamed through LDS in row tiles (nmfx_hals_wide_run) ------------------------------
// The sweep of hals_sweep_kernel at kp = 256, 384, .. 1024, where the kp x kp copy of G no longer fits in LDS (256 KiB at kp = 256).
// One wavefront still owns one problem, variable i on lane i % 64, slot i / 64 (NV = kp / 64 per lane), with the kept residual, the
// bound -x and 1 / G_jj (read once per launch from the diagonal in global memory) in registers; step j is the step above.  G
// reaches the waves in tiles of T rows, T kp 4 B <= 64 KiB: the block stages rows j0 .. j0 + T - 1 (2 lambda on the diagonal as
// it is staged) and each of its eight waves consumes them for its own problem -- once for the mat-vec, then once per sweep, the
// rows in ascending order: the update order is the definition's, x_0 .. x_{j-1} are new when step j runs.  T divides 64, so a
// tile's rows belong to one slot and the slot loop unrolls.
// The tile hand-over needs two block barriers per tile, so every loop around them is BLOCK-UNIFORM: the trip count of the loop over
// the problems is computed from nprob and the grid alone, every wave makes every trip, and a wave whose problem index is at or
// beyond nprob works on zeros and skips only its global loads and stores.  The early return on st->flag is grid-uniform and
// stands in front of the first barrier.  No atomics, a fixed order of every sum: two runs give the same bits.
template <int KP>
__global__ __launch_bounds__(64 * NMFX_HALS_WAVES) void hals_wide_sweep_kernel(
    const float* __restrict__ G, float diag_add, const float* __restrict__ R, float* __restrict__ X,
    int64_t sj, int64_t sc, int64_t nprob, int k, int sweeps, const DevState* __restrict__ st)
{
    if (st->flag) return;                               // (the stop rule has fired: the iterate stays; the same word for every block)
    constexpr int NV = KP / 64;                         // variables per lane
    constexpr int NW = NMFX_HALS_WAVES;
    constexpr int T = KP <= 256 ? 64 : KP <= 512 ? 32 : 16;      // rows of a tile
    static_assert(KP % 128 == 0 && KP >= 256 && KP <= 1024 && T * KP * 4 <= 65536 && (T * KP / 4) % (64 * NW) == 0, "tile");
    extern __shared__ __attribute__((aligned(16))) float hals_tile[];   // rows j0 .. j0 + T - 1 of G + diag_add I, [T][KP]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    bool valid[NV], live[NV]; float inv[NV];
#pragma unroll
    for (int t = 0; t < NV; ++t) {
        const int idx = lane + 64 * t;                  // (< KP)
        valid[t] = idx < k;
        const float gd = G[(int64_t)idx * KP + idx] + diag_add;
        live[t] = valid[t] && gd > 0.f;
        inv[t] = live[t] ? 1.f / gd : 0.f;
    }
    const int64_t per_trip = (int64_t)gridDim.x * NW;
    const int64_t trips = (nprob + per_trip - 1) / per_trip;            // (the same for every block)
    for (int64_t trip = 0; trip < trips; ++trip) {
        const int64_t c = trip * per_trip + (int64_t)blockIdx.x * NW + wave;
        const bool mine = c < nprob;                    // (wave-uniform; decides loads and stores only)
        float x[NV], g[NV], nx[NV];
#pragma unroll
        for (int t = 0; t < NV; ++t) {
            const int64_t off = (int64_t)(lane + 64 * t) * sj + c * sc;
            x[t] = (mine && valid[t]) ? X[off] : 0.f;
            g[t] = (mine && valid[t]) ? R[off] : 0.f;
            nx[t] = live[t] ? -x[t] : 0.f;              // the lower bound of a step, max(-x_j, .); 0 with inv = 0 where G_jj = 0: a step of 0
        }
        auto matvec = [&](int t2, int l, const float (&col)[NV]) {
            const float xl = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x[t2]), l));
#pragma unroll
            for (int t = 0; t < NV; ++t) g[t] = fmaf(-col[t], xl, g[t]);
        };
        auto step = [&](int t2, int j, const float (&col)[NV]) {
            const float cand = fmaxf(nx[t2], g[t2] * inv[t2]);
            const float d = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(cand), j));
            nx[t2] = (lane == j) ? nx[t2] - d : nx[t2];          // (d = -x_j: an exact zero)
#pragma unroll
            for (int t = 0; t < NV; ++t) g[t] = fmaf(-col[t], d, g[t]);
        };
        auto row = [&](int jj, float (&out)[NV]) {      // this lane's entries of row jj of the tile
#pragma unroll
            for (int t = 0; t < NV; ++t) out[t] = hals_tile[jj * KP + lane + 64 * t];
        };
        // one pass over the rows 0 .. k - 1 of G, tile by tile: op(slot, lane of the row's variable, the row)
        auto pass = [&](auto&& op) {
#pragma unroll
            for (int t2 = 0; t2 < NV; ++t2) {
                for (int j0 = 64 * t2; j0 < 64 * t2 + 64 && j0 < k; j0 += T) {       // (k: block-uniform)
                    __syncthreads();                    // every wave has consumed the tile before
                    for (int i4 = threadIdx.x; i4 < T * KP / 4; i4 += 64 * NW) {
                        float4 v = *reinterpret_cast<const float4*>(G + (int64_t)j0 * KP + 4 * (int64_t)i4);     // (j0 + T <= KP)
                        const int r = j0 + (4 * i4) / KP, col = (4 * i4) % KP;
                        v.x += (col == r) ? diag_add : 0.f; v.y += (col + 1 == r) ? diag_add : 0.f;
                        v.z += (col + 2 == r) ? diag_add : 0.f; v.w += (col + 3 == r) ? diag_add : 0.f;
                        *reinterpret_cast<float4*>(hals_tile + 4 * i4) = v;
                    }
                    __syncthreads();
                    const int lim = k - j0 < T ? k - j0 : T, l0 = j0 - 64 * t2;
                    int j = 0;
                    for (; j + 4 <= lim; j += 4) {       // four rows at a time: four LDS reads in flight together
                        float c0[NV], c1[NV], c2[NV], c3[NV];
                        row(j, c0); row(j + 1, c1); row(j + 2, c2); row(j + 3, c3);
                        op(t2, l0 + j, c0); op(t2, l0 + j + 1, c1); op(t2, l0 + j + 2, c2); op(t2, l0 + j + 3, c3);
                    }
                    for (; j < lim; ++j) {
                        float c0[NV];
                        row(j, c0);
                        op(t2, l0 + j, c0);
                    }
                }
            }
        };
        pass(matvec);                                   // g = r - G x
        for (int s = 0; s < sweeps; ++s) pass(step);
        if (mine) {
#pragma unroll
            for (int t = 0; t < NV; ++t)
                X[(int64_t)(lane + 64 * t) * sj + c * sc] = live[t] ? 0.f - nx[t] : x[t];      // (0 - 0: +0; padded lanes hold x = 0)
        }
    }
}

template <int KP>
static int launch_hals_wide_sweep(nmfx_engine* E, const float* G, float diag_add, const float* R, float* X, int64_t sj, int64_t sc,
                                  int64_t nprob, int sweeps) {
    int rc;
    const size_t shm = (size_t)(KP <= 256 ? 64 : KP <= 512 ? 32 : 16) * KP * sizeof(float);
    auto kern = hals_wide_sweep_kernel<KP>;
    if ((rc = nmfx_allow_lds(E, reinterpret_cast<const void*>(kern), (int)shm))) return rc;
    const int64_t blocks_needed = (nprob + NMFX_HALS_WAVES - 1) / NMFX_HALS_WAVES;
    const int64_t round = (int64_t)E->ncu * NMFX_HALS_BLOCKS_PER_CU;      // (a tile is at most 64 KiB: two blocks per CU)
    const unsigned grid = (unsigned)(blocks_needed < round ? blocks_needed : round);
    hipLaunchKernelGGL(kern, dim3(grid), dim3(64 * NMFX_HALS_WAVES), shm, E->stream, G, diag_add, R, X, sj, sc, nprob, E->k, sweeps,
                       E->state);
    NMFX_HIP(hipGetLastError());
    return NMFX_OK;
}

// Arguments and strides as nmfx_hals_sweep.  kp = 1024 is the last rank whose kept values fit the registers of a wave
// (about 4 NV VGPRs, plus NV per row of G in flight): nothing beyond it is instantiated.
int nmfx_hals_wide_sweep(nmfx_engine* E, const float* G, float diag_add, const float* R, float* X, int64_t sj, int64_t sc,
                         int64_t nprob, int sweeps) {
    ProfScope ps(E, "hals_sweep");
    ProfScope side(E, sc == 1 ? "hals_sweep_h" : "hals_sweep_w");
    if (nprob <= 0) return NMFX_OK;
    switch (E->kp) {
        case 256: return launch_hals_wide_sweep<256>(E, G, diag_add, R, X, sj, sc, nprob, sweeps);
        case 384: return launch_hals_wide_sweep<384>(E, G, diag_add, R, X, sj, sc, nprob, sweeps);
        case 512: return launch_hals_wide_sweep<512>(E, G, diag_add, R, X, sj, sc, nprob, sweeps);
        case 640: return launch_hals_wide_sweep<640>(E, G, diag_add, R, X, sj, sc, nprob, sweeps);
        case 768: return launch_hals_wide_sweep<768>(E, G, diag_add, R, X, sj, sc, nprob, sweeps);
        case 896: return launch_hals_wide_sweep<896>(E, G, diag_add, R, X, sj, sc, nprob, sweeps);
        case 1024: return launch_hals_wide_sweep<1024>(E, G, diag_add, R, X, sj, sc, nprob, sweeps);
    }
    E->err = "hals_wide_sweep: serves kp = 256, 384, .. 1024 (128 < k <= 1024 components)";
    return NMFX_E_ARG;
}

// ---- the per-column solve of the dense fold-in (nmfx_hals_foldin_dense_run) ---------------------------------------
// The layout, the staging and the step of hals_sweep_kernel -- a column that runs s <= 16 sweeps leaves the bits of the sweep kernel
// with sweeps = s -- with the stop rule of sp_hals_solve (kernels_sparse.hip) per column: after sweep s, d_s is the running max |delta|
// of the sweep (delta comes from v_readlane and is wave-uniform) and xmax_s the largest component (a dead component keeps its value
// and counts, padding does not; reduced over the wave, made uniform by v_readfirstlane); the column stops after the first s with
// d_s <= tol xmax_s, or at max_sweeps.  Before the sweeps 17, 33, ... the kept residual is formed anew: r is reloaded from R and the
// mat-vec redone.  Lane 0 writes the column's sweep count.  Behind the staging barrier there is no block barrier (the trip counts
// differ per wave); every loop bound and every exit is wave-uniform and the sweep loop is bounded by max_sweeps; the waves take
// the columns at a static stride: no atomics, two runs give the same bits.
template <int KP>
__global__ __launch_bounds__(64 * NMFX_HALS_WAVES) void hals_solve_kernel(
    const float* __restrict__ G, float diag_add, const float* __restrict__ R, float* __restrict__ X,
    int64_t sj, int64_t sc, int64_t nprob, int k, float tol, int max_sweeps, int32_t* __restrict__ counts,
    const DevState* __restrict__ st)
{
    if (st->flag) return;                               // (the stop rule has fired: the iterate stays, as in hals_sweep_kernel)
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
            nx[t] = live[t] ? -x[t] : 0.f;
        }
        auto matvec = [&](int t2, int l, const float (&col)[NV]) {
            const float xl = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x[t2]), l));
#pragma unroll
            for (int t = 0; t < NV; ++t) g[t] = fmaf(-col[t], xl, g[t]);
        };
        float dmax;                                     // the running max |delta| of the sweep (wave-uniform)
        auto step = [&](int t2, int j, const float (&col)[NV]) {
            const float cand = fmaxf(nx[t2], g[t2] * inv[t2]);
            const float d = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(cand), j));
            dmax = fmaxf(dmax, fabsf(d));
            nx[t2] = (lane == j) ? nx[t2] - d : nx[t2];          // (d = -x_j: an exact zero)
#pragma unroll
            for (int t = 0; t < NV; ++t) g[t] = fmaf(-col[t], d, g[t]);
        };
        // g -= G x, four rows at a time as in hals_sweep_kernel
        auto residual = [&]() {
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
        };
        residual();
        int s = 0;
        for (;;) {                                      // (bounded by max_sweeps)
            dmax = 0.f;
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
            ++s;
            float xmax = 0.f;                           // (a dead component keeps its value and counts; padding holds x = 0)
#pragma unroll
            for (int t = 0; t < NV; ++t) xmax = fmaxf(xmax, live[t] ? 0.f - nx[t] : x[t]);
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) xmax = fmaxf(xmax, __shfl_xor(xmax, off, 64));
            xmax = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(xmax)));
            const float dm = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(dmax)));
            if (dm <= tol * xmax || s >= max_sweeps) break;
            if ((s & 15) == 0) {                        // the kept residual anew: r from global memory, the mat-vec again
#pragma unroll
                for (int t = 0; t < NV; ++t) {
                    x[t] = live[t] ? 0.f - nx[t] : x[t];
                    g[t] = valid[t] ? R[(int64_t)at[t] * sj + c * sc] : 0.f;
                }
                residual();
            }
        }
#pragma unroll
        for (int t = 0; t < NV; ++t)
            if (lane + 64 * t < KP) X[(int64_t)at[t] * sj + c * sc] = live[t] ? 0.f - nx[t] : x[t];      // (0 - 0: +0; invalid lanes hold x = 0)
        if (lane == 0) counts[c] = s;
    }
}

template <int KP>
static int launch_hals_solve(nmfx_engine* E, const float* G, float diag_add, const float* R, float* X, int64_t sj, int64_t sc,
                             int64_t nprob, float tol, int max_sweeps, int32_t* counts) {
    int rc;
    const size_t shm = (size_t)KP * KP * sizeof(float);
    auto kern = hals_solve_kernel<KP>;
    if ((rc = nmfx_allow_lds(E, reinterpret_cast<const void*>(kern), (int)shm))) return rc;
    const int64_t blocks_needed = (nprob + NMFX_HALS_WAVES - 1) / NMFX_HALS_WAVES;
    const int64_t round = (int64_t)E->ncu * NMFX_HALS_BLOCKS_PER_CU;
    const unsigned grid = (unsigned)(blocks_needed < round ? blocks_needed : round);
    hipLaunchKernelGGL(kern, dim3(grid), dim3(64 * NMFX_HALS_WAVES), shm, E->stream, G, diag_add, R, X, sj, sc, nprob, E->k, tol,
                       max_sweeps, counts, E->state);
    NMFX_HIP(hipGetLastError());
    return NMFX_OK;
}

// the one kp dispatch of the solve; arguments and strides as nmfx_hals_sweep, counts: [nprob]
int nmfx_hals_solve(nmfx_engine* E, const float* G, float diag_add, const float* R, float* X, int64_t sj, int64_t sc,
                    int64_t nprob, float tol, int max_sweeps, int32_t* counts) {
    ProfScope ps(E, "hals_solve");
    if (nprob <= 0) return NMFX_OK;
    switch (E->kp) {
        case 16: return launch_hals_solve<16>(E, G, diag_add, R, X, sj, sc, nprob, tol, max_sweeps, counts);
        case 32: return launch_hals_solve<32>(E, G, diag_add, R, X, sj, sc, nprob, tol, max_sweeps, counts);
        case 64: return launch_hals_solve<64>(E, G, diag_add, R, X, sj, sc, nprob, tol, max_sweeps, counts);
        case 128: return launch_hals_solve<128>(E, G, diag_add, R, X, sj, sc, nprob, tol, max_sweeps, counts);
    }
    E->err = nmfx_small_k_text("hals_solve");
    return NMFX_E_ARG;
}

// ---- the stack's state and objective ------------------------------------------------------------------------------------------
// obj_p = 1/2 ||V||^2 - sum_{c in p} sum_i W_ic A_ic + 1/2 <(W^T W)_pp, (H H^T)_pp>,  A = V H^T (the summed right-hand sides of the W
// half-step that follows).  Everything below is f64 over the f32 values of W, H and A, in a fixed order, without atomics:
//   stack_colsum_kernel   per component, sum_i W_ic A_ic over fixed row slabs
//   stack_gram_kernel     the 16 x 16 tiles of W^T W / H H^T that hold entries of one problem, over fixed row / column slabs
//   stack_reduce_kernel   the slabs summed in slab order
//   stack_record_kernel   one block: per problem the two sums, obj[P j + p], the stop rule; `flag` once all have stopped
#define NMFX_STACK_CS_MAX 256             // row slabs of the column sums
#define NMFX_STACK_GS_MAX 32              // slabs of a Gram matrix
// layout of E->stack_part (doubles): [CS_MAX][kp] | [2][GS_MAX][kp kp] | col64 [kp] | gram64 [2][kp kp] | vv partials [1024]
struct StackPart { double *cs, *gs, *col, *gram, *vv; };
static StackPart stack_part(const nmfx_engine* E) {
    const int64_t kp = E->kp, kk = kp * kp;
    StackPart p;
    p.cs = E->stack_part; p.gs = p.cs + NMFX_STACK_CS_MAX * kp; p.col = p.gs + 2 * NMFX_STACK_GS_MAX * kk; p.gram = p.col + kp; p.vv = p.gram + 2 * kk;
    return p;
}
static int64_t stack_part_size(const nmfx_engine* E) { const int64_t kp = E->kp, kk = kp * kp; return NMFX_STACK_CS_MAX * kp + 2 * NMFX_STACK_GS_MAX * kk + kp + 2 * kk + 1024; }
static int64_t stack_slab_rows(int64_t rows, int max_slabs) { int64_t r = (rows + max_slabs - 1) / max_slabs; return (r + 63) / 64 * 64; }

__global__ void stack_reset_kernel(HalsStackDev* sk) {
    const int p = threadIdx.x;
    if (p < NMFX_STACK_MAX) { sk->pflag[p] = 0; sk->pstop_i[p] = -1; sk->pn_obj[p] = 0; }
}

struct StackLam { float w[NMFX_STACK_MAX]; float h[NMFX_STACK_MAX]; };      // (float)(2 lambda_p), as nmfx_hals_run forms its diag_add
__global__ void stack_lambda_kernel(HalsStackDev* sk, StackLam lam) {
    const int c = threadIdx.x;
    if (c >= NMFX_STACK_MAX) return;
    const unsigned p = sk->c2p[c];
    sk->diag[0][c] = p != NMFX_STACK_NONE ? lam.w[p] : 0.f;
    sk->diag[1][c] = p != NMFX_STACK_NONE ? lam.h[p] : 0.f;
}

// sum of squares of V [rows][ld] in f64: block b sums the elements b, b + blocks, ... of its threads' strides, a fixed order
__global__ __launch_bounds__(256) void stack_vv_kernel(const float* __restrict__ V, int64_t count, double* __restrict__ part) {
    __shared__ double sh[256];
    double s = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (int64_t)gridDim.x * 256) { const double v = (double)V[i]; s = fma(v, v, s); }
    sh[threadIdx.x] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) { if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w]; __syncthreads(); }
    if (threadIdx.x == 0) part[blockIdx.x] = sh[0];
}
__global__ __launch_bounds__(256) void stack_vv_sum_kernel(const double* __restrict__ part, int n, HalsStackDev* sk) {
    __shared__ double sh[256];
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) s += part[i];
    sh[threadIdx.x] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) { if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w]; __syncthreads(); }
    if (threadIdx.x == 0) sk->half_vv = 0.5 * sh[0];
}

// part[slab][c] = sum over the slab's rows of W[i][c] A[i][c]; thread = (row lane, column), the row lanes added in lane order
__global__ __launch_bounds__(256) void stack_colsum_kernel(const float* __restrict__ W, const float* __restrict__ A, int64_t rows, int64_t rps,
                                                           int kp, double* __restrict__ part, const DevState* __restrict__ st) {
    if (st->flag) return;
    __shared__ double sh[256];
    const int c = threadIdx.x % kp, rl = threadIdx.x / kp, nrl = 256 / kp;
    const int64_t r0 = (int64_t)blockIdx.x * rps, r1 = r0 + rps < rows ? r0 + rps : rows;
    double s = 0.0;
    for (int64_t r = r0 + rl; r < r1; r += nrl) s = fma((double)W[r * kp + c], (double)A[r * kp + c], s);
    sh[threadIdx.x] = s;
    __syncthreads();
    if (rl == 0) {
        for (int q = 1; q < nrl; ++q) s += sh[q * kp + c];
        part[(int64_t)blockIdx.x * kp + c] = s;
    }
}

// part[slab][a][b] = sum over the slab of F_a F_b for the 16 x 16 tiles (ta <= tb) that hold a pair of components of one problem.
// HSIDE: F = H [kp][ld], summed over columns; else F = W [rows][kp], summed over rows.
template <bool HSIDE>
__global__ __launch_bounds__(256) void stack_gram_kernel(const float* __restrict__ F, int64_t ld, int64_t rows, int64_t rps, int kp,
                                                         double* __restrict__ part, const HalsStackDev* __restrict__ sk,
                                                         const DevState* __restrict__ st) {
    if (st->flag) return;
    const int T = kp / 16, ta = blockIdx.y / T, tb = blockIdx.y % T;
    if (ta > tb) return;
    if (ta != tb) { const unsigned pa = sk->c2p[16 * ta + 15]; if (pa == NMFX_STACK_NONE || pa != sk->c2p[16 * tb]) return; }
    else if (sk->c2p[16 * ta] == NMFX_STACK_NONE) return;
    __shared__ double sa[64][17], sb[64][17];
    const int a = threadIdx.x >> 4, b = threadIdx.x & 15;
    const int64_t r0 = (int64_t)blockIdx.x * rps, r1 = r0 + rps < rows ? r0 + rps : rows;
    double acc = 0.0;
    for (int64_t rc = r0; rc < r1; rc += 64) {          // (rows and rps are multiples of 64)
        for (int e = threadIdx.x; e < 1024; e += 256) {
            int r, c;
            if (HSIDE) { r = e & 63; c = e >> 6; } else { c = e & 15; r = e >> 4; }
            const int64_t ia = HSIDE ? (int64_t)(16 * ta + c) * ld + rc + r : (rc + r) * (int64_t)kp + 16 * ta + c;
            const int64_t ib = HSIDE ? (int64_t)(16 * tb + c) * ld + rc + r : (rc + r) * (int64_t)kp + 16 * tb + c;
            sa[r][c] = (double)F[ia]; sb[r][c] = (double)F[ib];
        }
        __syncthreads();
#pragma unroll 8
        for (int r = 0; r < 64; ++r) acc = fma(sa[r][a], sb[r][b], acc);
        __syncthreads();
    }
    part[(int64_t)blockIdx.x * kp * kp + (int64_t)(16 * ta + a) * kp + 16 * tb + b] = acc;
}

// y = 0, 1: gram64[y][e] = the slabs of Gram y summed in slab order; y = 2: col64[c] likewise
__global__ __launch_bounds__(256) void stack_reduce_kernel(const double* __restrict__ cs, int ncs, const double* __restrict__ gs, int ngw, int ngh,
                                                           int kp, double* __restrict__ col, double* __restrict__ gram,
                                                           const DevState* __restrict__ st) {
    if (st->flag) return;
    const int e = blockIdx.x * 256 + threadIdx.x, kk = kp * kp;
    if (blockIdx.y == 2) {
        if (e >= kp) return;
        double s = 0.0;
        for (int q = 0; q < ncs; ++q) s += cs[(int64_t)q * kp + e];
        col[e] = s;
        return;
    }
    if (e >= kk) return;
    const double* src = gs + (int64_t)blockIdx.y * NMFX_STACK_GS_MAX * kk;
    const int n = blockIdx.y ? ngh : ngw;
    double s = 0.0;
    for (int q = 0; q < n; ++q) s += src[(int64_t)q * kk + e];
    gram[(int64_t)blockIdx.y * kk + e] = s;
}

__global__ __launch_bounds__(256) void stack_record_kernel(HalsStackDev* sk, const double* __restrict__ col, const double* __restrict__ gram, int kp,
                                                           double* __restrict__ obj_hist, int record, long long j, long long min_iter, double tol1,
                                                           double tol2, DevState* st) {
    if (st->flag) return;
    __shared__ double sh[256];
    const int P = sk->nprob, kk = kp * kp;
    int running = 0;
    for (int p = 0; p < P; ++p) {
        const int o = sk->off[p], kq = sk->off[p + 1] - o;
        double s = 0.0;
        for (int e = threadIdx.x; e < kq * kq; e += 256) {
            int a = o + e / kq, b = o + e % kq;
            if ((a >> 4) > (b >> 4)) { const int t = a; a = b; b = t; }      // (the tiles with ta <= tb are the ones that exist)
            s = fma(gram[a * kp + b], gram[kk + a * kp + b], s);
        }
        sh[threadIdx.x] = s;
        __syncthreads();
        for (int w = 128; w > 0; w >>= 1) { if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w]; __syncthreads(); }
        if (threadIdx.x == 0) {
            double dot = 0.0;
            for (int c = o; c < o + kq; ++c) dot += col[c];
            const double whwh = sh[0];
            sk->terms[p][0] = dot; sk->terms[p][1] = whwh;
            if (record && !sk->pflag[p]) {              // the rule of nmfx_record_objective, on the problem's own history
                const double obj = (sk->half_vv - dot) + 0.5 * whwh;
                int rule = 0;
                if (j >= 1 && (j - 1) > min_iter) {
                    const double prev = obj_hist[(long long)P * (j - 1) + p];
                    if (obj < tol1) rule = 1;
                    else if (obj >= prev - tol2) rule = 2;
                }
                obj_hist[(long long)P * j + p] = obj;
                sk->pn_obj[p] = j + 1;
                if (rule) { sk->pflag[p] = rule; sk->pstop_i[p] = j - 1; }
            }
            if (!sk->pflag[p]) ++running;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0 && record && !running) { st->flag = 1; st->stop_i = j - 1; }
}

int nmfx_hals_stack_alloc(nmfx_engine* E) {
    int rc;
    if ((rc = nmfx_lazy_alloc(E, &E->stack_dev, 1))) return rc;
    return nmfx_lazy_alloc(E, &E->stack_part, stack_part_size(E));
}

int nmfx_hals_stack_config(nmfx_engine* E) {
    int rc;
    if ((rc = nmfx_hals_stack_alloc(E))) return rc;
    static_assert(offsetof(HalsStackDev, diag) > offsetof(HalsStackDev, pn_obj), "the configuration is the front of HalsStackDev");
    std::vector<char> buf(offsetof(HalsStackDev, diag), 0);
    HalsStackDev* h = reinterpret_cast<HalsStackDev*>(buf.data());      // (only the front is touched)
    h->nprob = E->stack_nprob;
    for (int p = 0; p <= NMFX_STACK_MAX; ++p) h->off[p] = E->stack_off[p <= E->stack_nprob ? p : E->stack_nprob];
    for (int c = 0; c < NMFX_STACK_MAX; ++c) h->c2p[c] = NMFX_STACK_NONE;
    for (int p = 0; p < E->stack_nprob; ++p)
        for (int c = E->stack_off[p]; c < E->stack_off[p + 1]; ++c) h->c2p[c] = (unsigned char)p;
    for (int p = 0; p < NMFX_STACK_MAX; ++p) { h->pflag[p] = 0; h->pstop_i[p] = -1; h->pn_obj[p] = 0; }
    NMFX_HIP(hipMemcpyAsync(E->stack_dev, buf.data(), buf.size(), hipMemcpyHostToDevice, E->stream));
    NMFX_HIP(hipStreamSynchronize(E->stream));
    return NMFX_OK;
}

int nmfx_hals_stack_reset(nmfx_engine* E) {
    if (!E->stack_dev) return NMFX_OK;
    hipLaunchKernelGGL(stack_reset_kernel, dim3(1), dim3(NMFX_STACK_MAX), 0, E->stream, E->stack_dev);
    NMFX_HIP(hipGetLastError());
    return NMFX_OK;
}

int nmfx_hals_stack_lambdas(nmfx_engine* E, const double* lambda_w, const double* lambda_h) {
    StackLam lam;
    for (int p = 0; p < NMFX_STACK_MAX; ++p) {
        lam.w[p] = p < E->stack_nprob ? (float)(2.0 * lambda_w[p]) : 0.f;
        lam.h[p] = p < E->stack_nprob ? (float)(2.0 * lambda_h[p]) : 0.f;
    }
    hipLaunchKernelGGL(stack_lambda_kernel, dim3(1), dim3(NMFX_STACK_MAX), 0, E->stream, E->stack_dev, lam);
    NMFX_HIP(hipGetLastError());
    return NMFX_OK;
}

int nmfx_hals_stack_vv(nmfx_engine* E) {
    if (E->stack_vv_ready) return NMFX_OK;
    int rc;
    if ((rc = nmfx_need_v(E))) return rc;
    const StackPart sp = stack_part(E);
    hipLaunchKernelGGL(stack_vv_kernel, dim3(1024), dim3(256), 0, E->stream, E->V, E->mp * E->np, sp.vv);
    hipLaunchKernelGGL(stack_vv_sum_kernel, dim3(1), dim3(256), 0, E->stream, sp.vv, 1024, E->stack_dev);
    NMFX_HIP(hipGetLastError());
    E->stack_vv_ready = true;
    return NMFX_OK;
}

int nmfx_hals_stack_ensure_obj(nmfx_engine* E, int64_t need) {
    if (need <= E->stack_obj_cap) return NMFX_OK;
    int64_t cap = E->stack_obj_cap ? E->stack_obj_cap : 8192;
    while (cap < need) cap *= 2;
    double* nbuf = nullptr;
    NMFX_HIP(hipMalloc(reinterpret_cast<void**>(&nbuf), (size_t)cap * sizeof(double)));
    NMFX_HIP(hipMemsetAsync(nbuf, 0, (size_t)cap * sizeof(double), E->stream));
    if (E->stack_obj) {
        NMFX_HIP(hipMemcpyAsync(nbuf, E->stack_obj, (size_t)E->stack_obj_cap * sizeof(double), hipMemcpyDeviceToDevice, E->stream));
        NMFX_HIP(hipStreamSynchronize(E->stream));
        NMFX_HIP(hipFree(E->stack_obj));
    }
    E->stack_obj = nbuf;
    E->stack_obj_cap = cap;
    return NMFX_OK;
}

int nmfx_hals_stack_objective(nmfx_engine* E, bool record, int64_t j, int64_t min_iter, double tol1, double tol2) {
    ProfScope ps(E, "stack_objective");
    const StackPart sp = stack_part(E);
    const int kp = E->kp, kk = kp * kp;
    const int64_t rps_c = stack_slab_rows(E->mp, NMFX_STACK_CS_MAX), rps_w = stack_slab_rows(E->mp, NMFX_STACK_GS_MAX),
                  rps_h = stack_slab_rows(E->np, NMFX_STACK_GS_MAX);
    const int ncs = (int)((E->mp + rps_c - 1) / rps_c), ngw = (int)((E->mp + rps_w - 1) / rps_w), ngh = (int)((E->np + rps_h - 1) / rps_h);
    const int T = kp / 16;
    hipLaunchKernelGGL(stack_colsum_kernel, dim3(ncs), dim3(256), 0, E->stream, E->W[0], E->Asum, E->mp, rps_c, kp, sp.cs, E->state);
    hipLaunchKernelGGL((stack_gram_kernel<false>), dim3(ngw, T * T), dim3(256), 0, E->stream, E->W[0], (int64_t)kp, E->mp, rps_w, kp, sp.gs,
                       E->stack_dev, E->state);
    hipLaunchKernelGGL((stack_gram_kernel<true>), dim3(ngh, T * T), dim3(256), 0, E->stream, E->H, E->np, E->np, rps_h, kp,
                       sp.gs + (int64_t)NMFX_STACK_GS_MAX * kk, E->stack_dev, E->state);
    hipLaunchKernelGGL(stack_reduce_kernel, dim3((kk + 255) / 256, 3), dim3(256), 0, E->stream, sp.cs, ncs, sp.gs, ngw, ngh, kp, sp.col, sp.gram,
                       E->state);
    hipLaunchKernelGGL(stack_record_kernel, dim3(1), dim3(256), 0, E->stream, E->stack_dev, sp.col, sp.gram, kp, E->stack_obj, record ? 1 : 0,
                       (long long)j, (long long)min_iter, tol1, tol2, E->state);
    NMFX_HIP(hipGetLastError());
    return NMFX_OK;
}

// (nmfx_create: forces this translation unit's code object onto the device under the library's start-up lock)
int nmfx_preload_hals() { hipFuncAttributes a; return hipFuncGetAttributes(&a, reinterpret_cast<const void*>(hals_sweep_kernel<128>)) == hipSuccess ? 0 : -1; }
