// HALS: hierarchical alternating least squares (Cichocki & Phan 2009; scikit-learn's solver = 'cd').
//
// A half-step works on the per-problem data of an ANLS half-step (kernels_anls.hip): the shared Gram matrix
// G = F^T F + 2 lambda I and one right-hand side r = F^T b per row of W / column of H.  Where ANLS solves every problem
// exactly, HALS makes `sweeps` projected Gauss-Seidel sweeps over the k components from the current solution x >= 0:
//     for j = 0 .. k-1:  if G_jj > 0:  x_j <- max(0, x_j + (r_j - sum_l G_jl x_l) / G_jj)      (x_0 .. x_{j-1} already new)
// A component with G_jj = 0 (dead, at lambda = 0) keeps its value.  The clamp is an exact zero.
//
// One wavefront owns one problem, variable i on lane i % 64, slot i / 64 (NV slots per lane).  The wave keeps the residual
// g = r - G x in registers: one mat-vec per problem, and step j is
//     delta = max(-x_j, g_j / G_jj) on lane j, broadcast (v_readlane);  x_j += delta;  g_i -= delta G_ij on every lane
// (the lane keeps -x_j, the lower bound of its step, instead of x_j)
// so that further sweeps need no new mat-vec.  G is symmetric, column j is row j: it is read from a copy in LDS that the block
// stages (2 lambda already on its diagonal), consecutive lanes on consecutive addresses.  Every loop bound is wave-uniform
// (k, sweeps, the problem index); there are no atomics, and the order of every sum is fixed: two runs give the same bits.  Rows,
// columns and lanes at or beyond k are never read into a sum; the padded variables are written back as exact zeros.
//
// Each piece of this is written once and the three kernels are shells over the pieces:
//   hals_stage      rows [j0, j0 + T) of G into LDS with the diagonal added (STACK: masked to the problems' diagonal blocks)
//   HalsLane        a lane's valid / live / 1 / G_jj, x, g and -x: set-up from the diagonal, load, matvec, step, value, store
//   hals_rows       a run of rows, four LDS reads in flight, then the tail: op(row index, the lane's entries of the row)
//   hals_problems   hals_sweep_kernel (kp <= 128, G whole in LDS; plain and STACK) and, with SOLVE, hals_solve_kernel: the same
//                   body with the per-column stop rule of the dense fold-in
//   hals_wide_sweep_kernel   kp = 256 .. 1024: G streamed through LDS in row tiles, two block barriers per tile
//   hals_launch     the LDS allowance and the grid of all three
#include "nmfx_internal.h"

#define NMFX_HALS_WAVES 8                 // problems a block works on at a time
#define NMFX_HALS_BLOCKS_PER_CU 2         // one round of the grid (the copy of G, or a tile of it, is at most 64 KiB: a CU holds two blocks)

// Rows [j0, j0 + T) of G [KP][KP] -> lds [T][KP], diag_add on the diagonal (j0 + T <= KP; the whole block calls, no barrier inside).
// STACK (nmfx_hals_stack_*): the k components are P problems side by side.  An entry whose row and column belong to different
// problems, or to none, is stored as zero and the diagonal gets its own problem's 2 lambda_p (sk->diag[side], 0 for a component
// of no problem) in place of diag_add: the sweep over the stacked components is then P independent sweeps -- a masked term is
// fmaf(-0 d, ., g) = g, bit for bit.
template <int KP, int T, bool STACK>
__device__ __forceinline__ void hals_stage(float* lds, const float* __restrict__ G, float diag_add, int j0,
                                           const HalsStackDev* __restrict__ sk = nullptr, int side = 0) {
    for (int i4 = threadIdx.x; i4 < T * KP / 4; i4 += 64 * NMFX_HALS_WAVES) {
        float4 v = *reinterpret_cast<const float4*>(G + (int64_t)j0 * KP + 4 * (int64_t)i4);
        const int row = j0 + (4 * i4) / KP, col = (4 * i4) % KP;
        float dg = diag_add;
        if constexpr (STACK) {
            const unsigned pr = sk->c2p[row];
            const unsigned pc4 = *reinterpret_cast<const unsigned*>(sk->c2p + col);       // (col is a multiple of 4)
            const bool own = pr != NMFX_STACK_NONE;
            v.x = (own && (pc4 & 255u) == pr) ? v.x : 0.f;          v.y = (own && ((pc4 >> 8) & 255u) == pr) ? v.y : 0.f;
            v.z = (own && ((pc4 >> 16) & 255u) == pr) ? v.z : 0.f;  v.w = (own && (pc4 >> 24) == pr) ? v.w : 0.f;
            dg = sk->diag[side][row];
        }
        v.x += (col == row) ? dg : 0.f; v.y += (col + 1 == row) ? dg : 0.f;
        v.z += (col + 2 == row) ? dg : 0.f; v.w += (col + 3 == row) ? dg : 0.f;
        *reinterpret_cast<float4*>(lds + 4 * i4) = v;
    }
}

// One lane's share of a wave's problem: variable at[t] = lane + 64 t in slot t.
template <int KP, int NV>
struct HalsLane {
    int lane, at[NV];                     // (lanes at or beyond KP at kp = 16 / 32: an address inside the row; their values are unused, never stored)
    bool valid[NV], live[NV];             // below k; and with G_jj > 0 (STACK: and owned by a problem that runs)
    float inv[NV];                        // 1 / G_jj, 0 where not live: a step of 0
    float x[NV], g[NV], nx[NV];           // x as loaded; the kept residual; -x, the lower bound of a step max(-x_j, .), 0 where not live

    __device__ __forceinline__ void init(int k) {
        lane = threadIdx.x & 63;
#pragma unroll
        for (int t = 0; t < NV; ++t) {
            const int idx = lane + 64 * t;
            valid[t] = idx < k;
            at[t] = idx < KP ? idx : KP - 1;
        }
    }
    // gd: the variable's diagonal entry of G + diag_add I
    __device__ __forceinline__ void set_diag(int t, float gd, bool runs = true) {
        live[t] = valid[t] && gd > 0.f && runs;
        inv[t] = live[t] ? 1.f / gd : 0.f;
    }
    __device__ __forceinline__ int64_t off(int t, int64_t sj, int64_t sc, int64_t c) const { return (int64_t)at[t] * sj + c * sc; }
    // `mine` (wave-uniform) guards the loads only: a wave without a problem works on zeros
    __device__ __forceinline__ void load_rhs(const float* __restrict__ R, int64_t sj, int64_t sc, int64_t c, bool mine = true) {
#pragma unroll
        for (int t = 0; t < NV; ++t) g[t] = (mine && valid[t]) ? R[off(t, sj, sc, c)] : 0.f;
    }
    __device__ __forceinline__ void load(const float* __restrict__ X, const float* __restrict__ R, int64_t sj, int64_t sc, int64_t c,
                                         bool mine = true) {
#pragma unroll
        for (int t = 0; t < NV; ++t) {
            const int64_t o = off(t, sj, sc, c);        // (a single offset per slot, used by both loads, keeps the VGPR count these kernels had before the pieces were shared)
            x[t] = (mine && valid[t]) ? X[o] : 0.f;
            g[t] = (mine && valid[t]) ? R[o] : 0.f;
            nx[t] = live[t] ? -x[t] : 0.f;
        }
    }
    // g -= G[:, l] x_l for variable l of slot t2: column l of G (= row l) against x_l, broadcast from its lane
    __device__ __forceinline__ void matvec(int t2, int l, const float (&row)[NV]) {
        const float xl = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x[t2]), l));
#pragma unroll
        for (int t = 0; t < NV; ++t) g[t] = fmaf(-row[t], xl, g[t]);
    }
    // THE step, of variable j of slot t2: every lane forms its own candidate from its current g, lane j's is the step.  Returns
    // delta (wave-uniform).
    __device__ __forceinline__ float step(int t2, int j, const float (&row)[NV]) {
        const float cand = fmaxf(nx[t2], g[t2] * inv[t2]);
        const float d = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(cand), j));
        nx[t2] = (lane == j) ? nx[t2] - d : nx[t2];              // (d = -x_j: an exact zero)
#pragma unroll
        for (int t = 0; t < NV; ++t) g[t] = fmaf(-row[t], d, g[t]);
        return d;
    }
    // the current x: 0 - 0 is +0, a variable that is not live is as it was read (a padded one: 0)
    __device__ __forceinline__ float value(int t) const { return live[t] ? 0.f - nx[t] : x[t]; }
    __device__ __forceinline__ void store(float* __restrict__ X, int64_t sj, int64_t sc, int64_t c) const {
#pragma unroll
        for (int t = 0; t < NV; ++t)
            if (lane + 64 * t < KP) X[off(t, sj, sc, c)] = value(t);
    }
};

// this lane's entries of row `j` of a staged [.][KP] block of G, at the lane's (clamped) columns at[]
template <int KP, int NV>
__device__ __forceinline__ void hals_row(const float* gs, int j, const int (&at)[NV], float (&out)[NV]) {
#pragma unroll
    for (int t = 0; t < NV; ++t) out[t] = gs[j * KP + at[t]];
}
// ... where no lane lies beyond KP (the wide kernel): column lane + 64 t, one base address and constant offsets
template <int KP, int NV>
__device__ __forceinline__ void hals_row(const float* gs, int j, int lane, float (&out)[NV]) {
#pragma unroll
    for (int t = 0; t < NV; ++t) out[t] = gs[j * KP + lane + 64 * t];
}

// op(l, row l) for l = 0 .. lim - 1, four rows at a time so that the four LDS reads are in flight together, then the tail
// (written out: v_readlane is convergent and the trip count is not a constant).  l stays a scalar loop counter; no barrier.
template <int NV, typename Read, typename Op>
__device__ __forceinline__ void hals_rows(int lim, Read&& read, Op&& op) {
    int l = 0;
    for (; l + 4 <= lim; l += 4) {
        float c0[NV], c1[NV], c2[NV], c3[NV];
        read(l, c0); read(l + 1, c1); read(l + 2, c2); read(l + 3, c3);
        op(l, c0); op(l + 1, c1); op(l + 2, c2); op(l + 3, c3);
    }
    for (; l < lim; ++l) {
        float c0[NV];
        read(l, c0);
        op(l, c0);
    }
}

// kp <= 128: the block stages G whole, once, and its waves loop over the problems at a static stride.  Behind the staging barrier
// there is no block barrier (with SOLVE the trip counts differ per wave).
// STACK: a component of a stopped problem, or of none, is not live: its steps are exact zeros and its x is written back as it was
// read.  The stop state is read once per launch, before the loop over the problems.
// SOLVE (the dense fold-in): `sweeps` is the cap, and a column stops after the first sweep s with d_s <= tol xmax_s,
// d_s the running max |delta| of the sweep (delta comes from v_readlane and is wave-uniform) and xmax_s the largest component (a
// dead component keeps its value and counts, padding does not; reduced over the wave, made uniform by v_readfirstlane).  Before the
// sweeps 17, 33, ... the kept residual is formed anew: r is reloaded from R and the mat-vec redone.  Lane 0 writes the column's sweep
// count.  Without SOLVE none of that is compiled, so a column that runs s <= 16 sweeps leaves the bits of the plain sweep.
template <int KP, bool STACK, bool SOLVE>
__device__ __forceinline__ void hals_problems(const float* __restrict__ G, float diag_add, const float* __restrict__ R, float* __restrict__ X,
                                              int64_t sj, int64_t sc, int64_t nprob, int k, int sweeps, float tol, int32_t* __restrict__ counts,
                                              const HalsStackDev* __restrict__ sk, int side)
{
    constexpr int NV = KP <= 64 ? 1 : KP / 64;          // variables per lane
    constexpr int NW = NMFX_HALS_WAVES;
    extern __shared__ __attribute__((aligned(16))) float hals_g[];      // G + diag_add I, [KP][KP]
    hals_stage<KP, KP, STACK>(hals_g, G, diag_add, 0, sk, side);
    __syncthreads();
    const int wave = threadIdx.x >> 6;
    HalsLane<KP, NV> S;
    S.init(k);
#pragma unroll
    for (int t = 0; t < NV; ++t) {
        bool runs = true;
        if constexpr (STACK) {
            const unsigned p = sk->c2p[S.at[t]];
            runs = p != NMFX_STACK_NONE && sk->pflag[p < NMFX_STACK_MAX ? p : 0] == 0;
        }
        S.set_diag(t, hals_g[S.at[t] * KP + S.at[t]], runs);
    }
    // one pass over the rows 0 .. k - 1 of G: op(slot, lane of the row's variable, the row)
    auto pass = [&](auto&& op) {
#pragma unroll
        for (int t2 = 0; t2 < NV; ++t2)
            hals_rows<NV>(k - 64 * t2 < 64 ? k - 64 * t2 : 64,
                          [&](int l, float (&row)[NV]) { hals_row<KP, NV>(hals_g, 64 * t2 + l, S.at, row); },
                          [&](int l, const float (&row)[NV]) { op(t2, l, row); });
    };
    auto matvec = [&](int t2, int l, const float (&row)[NV]) { S.matvec(t2, l, row); };
    for (int64_t c = (int64_t)blockIdx.x * NW + wave; c < nprob; c += (int64_t)gridDim.x * NW) {      // (wave-uniform)
        S.load(X, R, sj, sc, c);
        pass(matvec);                                   // g = r - G x
        int s = 0;
        while (SOLVE || s < sweeps) {                   // (SOLVE: left by the break below, at s = sweeps at the latest)
            [[maybe_unused]] float dmax = 0.f;
            pass([&](int t2, int j, const float (&row)[NV]) {
                [[maybe_unused]] const float d = S.step(t2, j, row);
                if constexpr (SOLVE) dmax = fmaxf(dmax, fabsf(d));
            });
            ++s;
            if constexpr (SOLVE) {
                float xmax = 0.f;
#pragma unroll
                for (int t = 0; t < NV; ++t) xmax = fmaxf(xmax, S.value(t));
#pragma unroll
                for (int off = 1; off < 64; off <<= 1) xmax = fmaxf(xmax, __shfl_xor(xmax, off, 64));
                xmax = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(xmax)));
                const float dm = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(dmax)));
                if (dm <= tol * xmax || s >= sweeps) break;
                if ((s & 15) == 0) {                    // the kept residual anew: r from global memory, the mat-vec again
#pragma unroll
                    for (int t = 0; t < NV; ++t) S.x[t] = S.value(t);
                    S.load_rhs(R, sj, sc, c);
                    pass(matvec);
                }
            }
        }
        S.store(X, sj, sc, c);
        if constexpr (SOLVE) { if (S.lane == 0) counts[c] = s; }
    }
}

template <int KP, bool STACK = false>
__global__ __launch_bounds__(64 * NMFX_HALS_WAVES) void hals_sweep_kernel(
    const float* __restrict__ G, float diag_add, const float* __restrict__ R, float* __restrict__ X,
    int64_t sj, int64_t sc, int64_t nprob, int k, int sweeps, const DevState* __restrict__ st,
    const HalsStackDev* __restrict__ sk = nullptr, int side = 0)
{
    if (st->flag) return;                               // (the stop rule has fired: the iterate stays)
    hals_problems<KP, STACK, false>(G, diag_add, R, X, sj, sc, nprob, k, sweeps, 0.f, nullptr, sk, side);
}

// the per-column solve of the dense fold-in (nmfx_hals_foldin_dense_run)
template <int KP>
__global__ __launch_bounds__(64 * NMFX_HALS_WAVES) void hals_solve_kernel(
    const float* __restrict__ G, float diag_add, const float* __restrict__ R, float* __restrict__ X,
    int64_t sj, int64_t sc, int64_t nprob, int k, float tol, int max_sweeps, int32_t* __restrict__ counts,
    const DevState* __restrict__ st)
{
    if (st->flag) return;                               // (as in hals_sweep_kernel)
    hals_problems<KP, false, true>(G, diag_add, R, X, sj, sc, nprob, k, max_sweeps, tol, counts, nullptr, 0);
}

// ---- beyond 128 components: G streamed through LDS in row tiles (nmfx_hals_wide_run) ------------------------------
// The sweep at kp = 256, 384, .. 1024, where the kp x kp copy of G no longer fits in LDS (256 KiB at kp = 256).  The lane state and
// the step are HalsLane's, with 1 / G_jj read once per launch from the diagonal in global memory.  G reaches the waves in tiles of
// T rows, T kp 4 B <= 64 KiB: the block stages rows j0 .. j0 + T - 1 and each of its eight waves consumes them for its own problem --
// once for the mat-vec, then once per sweep, the rows in ascending order: the update order is the definition's, x_0 .. x_{j-1} are
// new when step j runs.  T divides 64, so a tile's rows belong to one slot and the slot loop unrolls.
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
    const int wave = threadIdx.x >> 6;
    HalsLane<KP, NV> S;
    S.init(k);
#pragma unroll
    for (int t = 0; t < NV; ++t) S.set_diag(t, G[(int64_t)S.at[t] * KP + S.at[t]] + diag_add);
    const int64_t per_trip = (int64_t)gridDim.x * NW;
    const int64_t trips = (nprob + per_trip - 1) / per_trip;            // (the same for every block)
    for (int64_t trip = 0; trip < trips; ++trip) {
        const int64_t c = trip * per_trip + (int64_t)blockIdx.x * NW + wave;
        const bool mine = c < nprob;                    // (wave-uniform; decides loads and stores only)
        S.load(X, R, sj, sc, c, mine);
        // one pass over the rows 0 .. k - 1 of G, tile by tile: op(slot, lane of the row's variable, the row)
        auto pass = [&](auto&& op) {
#pragma unroll
            for (int t2 = 0; t2 < NV; ++t2) {
                for (int j0 = 64 * t2; j0 < 64 * t2 + 64 && j0 < k; j0 += T) {       // (k: block-uniform)
                    __syncthreads();                    // every wave has consumed the tile before
                    hals_stage<KP, T, false>(hals_tile, G, diag_add, j0);
                    __syncthreads();
                    const int l0 = j0 - 64 * t2;
                    hals_rows<NV>(k - j0 < T ? k - j0 : T,
                                  [&](int j, float (&row)[NV]) { hals_row<KP, NV>(hals_tile, j, S.lane, row); },
                                  [&](int j, const float (&row)[NV]) { op(t2, l0 + j, row); });
                }
            }
        };
        pass([&](int t2, int l, const float (&row)[NV]) { S.matvec(t2, l, row); });      // g = r - G x
        for (int s = 0; s < sweeps; ++s) pass([&](int t2, int j, const float (&row)[NV]) { S.step(t2, j, row); });
        if (mine) S.store(X, sj, sc, c);
    }
}

// ---- launches ------------------------------------------------------------------------------------------------------------------
// One family of problems: the arguments every kernel above starts with.  Strides as the NNLS launcher of kernels_anls.hip
// (W: sj = 1, sc = kp; H: sj = np, sc = 1).
struct HalsSys { const float* G; float diag_add; const float* R; float* X; int64_t sj, sc, nprob; };

// the LDS allowance and the grid of every kernel above; `rest`: the kernel's arguments behind k
template <typename K, typename... A>
static int hals_launch(nmfx_engine* E, K kern, size_t shm, const HalsSys& p, A... rest) {
    int rc;
    if ((rc = nmfx_allow_lds(E, reinterpret_cast<const void*>(kern), (int)shm))) return rc;
    const int64_t blocks_needed = (p.nprob + NMFX_HALS_WAVES - 1) / NMFX_HALS_WAVES;
    const int64_t round = (int64_t)E->ncu * NMFX_HALS_BLOCKS_PER_CU;
    const unsigned grid = (unsigned)(blocks_needed < round ? blocks_needed : round);
    hipLaunchKernelGGL(kern, dim3(grid), dim3(64 * NMFX_HALS_WAVES), shm, E->stream, p.G, p.diag_add, p.R, p.X, p.sj, p.sc, p.nprob, E->k,
                       rest...);
    NMFX_HIP(hipGetLastError());
    return NMFX_OK;
}

// the one kp dispatch of the kernels that hold G whole: launch(the constant KP, the bytes of LDS)
template <typename F>
static int hals_small_kp(nmfx_engine* E, const char* who, F&& launch) {
    const size_t shm = (size_t)E->kp * E->kp * sizeof(float);
    switch (E->kp) {
        case 16: return launch(std::integral_constant<int, 16>(), shm);
        case 32: return launch(std::integral_constant<int, 32>(), shm);
        case 64: return launch(std::integral_constant<int, 64>(), shm);
        case 128: return launch(std::integral_constant<int, 128>(), shm);
    }
    E->err = nmfx_small_k_text(who);
    return NMFX_E_ARG;
}

// stack_side >= 0: the stacked form (nmfx_internal.h); its diagonal comes from the stack's own lambdas, not from diag_add.
int nmfx_hals_sweep(nmfx_engine* E, const float* G, float diag_add, const float* R, float* X, int64_t sj, int64_t sc,
                    int64_t nprob, int sweeps, int stack_side) {
    ProfScope ps(E, "hals_sweep");
    ProfScope side(E, sc == 1 ? "hals_sweep_h" : "hals_sweep_w");          // (the same launch under its side's name: tools/hals_transform_perf.py --dense)
    if (nprob <= 0) return NMFX_OK;
    if (stack_side < 0)
        return hals_small_kp(E, "hals_sweep", [&](auto kp, size_t shm) {
            return hals_launch(E, hals_sweep_kernel<decltype(kp)::value, false>, shm, HalsSys{G, diag_add, R, X, sj, sc, nprob}, sweeps, E->state,
                               (const HalsStackDev*)nullptr, 0);
        });
    return hals_small_kp(E, "hals_stack_sweep", [&](auto kp, size_t shm) {
        return hals_launch(E, hals_sweep_kernel<decltype(kp)::value, true>, shm, HalsSys{G, 0.f, R, X, sj, sc, nprob}, sweeps, E->state,
                           (const HalsStackDev*)E->stack_dev, stack_side);
    });
}

// counts: [nprob]
int nmfx_hals_solve(nmfx_engine* E, const float* G, float diag_add, const float* R, float* X, int64_t sj, int64_t sc,
                    int64_t nprob, float tol, int max_sweeps, int32_t* counts) {
    ProfScope ps(E, "hals_solve");
    if (nprob <= 0) return NMFX_OK;
    return hals_small_kp(E, "hals_solve", [&](auto kp, size_t shm) {
        return hals_launch(E, hals_solve_kernel<decltype(kp)::value>, shm, HalsSys{G, diag_add, R, X, sj, sc, nprob}, tol, max_sweeps, counts,
                           E->state);
    });
}

template <int KP>
static int launch_hals_wide_sweep(nmfx_engine* E, const HalsSys& p, int sweeps) {
    return hals_launch(E, hals_wide_sweep_kernel<KP>, (size_t)(KP <= 256 ? 64 : KP <= 512 ? 32 : 16) * KP * sizeof(float), p, sweeps, E->state);
}

// kp = 1024 is the last rank whose kept values fit the registers of a wave (about 4 NV VGPRs, plus NV per row of G in flight):
// nothing beyond it is instantiated.
int nmfx_hals_wide_sweep(nmfx_engine* E, const float* G, float diag_add, const float* R, float* X, int64_t sj, int64_t sc,
                         int64_t nprob, int sweeps) {
    ProfScope ps(E, "hals_sweep");
    ProfScope side(E, sc == 1 ? "hals_sweep_h" : "hals_sweep_w");
    if (nprob <= 0) return NMFX_OK;
    const HalsSys p{G, diag_add, R, X, sj, sc, nprob};
    switch (E->kp) {
        case 256: return launch_hals_wide_sweep<256>(E, p, sweeps);
        case 384: return launch_hals_wide_sweep<384>(E, p, sweeps);
        case 512: return launch_hals_wide_sweep<512>(E, p, sweeps);
        case 640: return launch_hals_wide_sweep<640>(E, p, sweeps);
        case 768: return launch_hals_wide_sweep<768>(E, p, sweeps);
        case 896: return launch_hals_wide_sweep<896>(E, p, sweeps);
        case 1024: return launch_hals_wide_sweep<1024>(E, p, sweeps);
    }
    E->err = "hals_wide_sweep: serves kp = 256, 384, .. 1024 (128 < k <= 1024 components)";
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
