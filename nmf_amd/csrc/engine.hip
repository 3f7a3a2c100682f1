// C ABI of libnmfx.so: handle lifecycle, data movement, iteration state.
#include "nmfx_internal.h"
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <tuple>
#include <mutex>
#include <utility>

int nmfx_mur_eu_phase_a(nmfx_engine* E, double lambda_w, int64_t j);
int nmfx_mur_eu_phase_b(nmfx_engine* E, double lambda_h, int64_t min_iter, double tol1, double tol2, int64_t j);
int nmfx_mur_eu_finish_a(nmfx_engine* E, int64_t j);
int nmfx_mur_kl_phase_a(nmfx_engine* E, double lambda_w, int64_t j);
int nmfx_mur_kl_phase_b(nmfx_engine* E, double lambda_h, int64_t min_iter, double tol1, double tol2, int64_t j);
int nmfx_mur_kl_finish_a(nmfx_engine* E, int64_t j);

#ifndef NMFX_DEFAULT_PRECISION
#define NMFX_DEFAULT_PRECISION 1   /* split bf16 where available (k padded to 64, MUR-eu); NMFX_PRECISION=f32 for exact f32 */
#endif
static thread_local std::string g_err;

int nmfx_allow_lds(nmfx_engine* E, const void* kernel, int bytes) {
    if (bytes <= 64 * 1024) return NMFX_OK;            // within the default limit
    static std::mutex mu;
    static std::map<std::pair<int, const void*>, int> granted;
    std::lock_guard<std::mutex> lock(mu);
    int& have = granted[std::make_pair(E->device, kernel)];
    if (have >= bytes) return NMFX_OK;
    NMFX_HIP(hipSetDevice(E->device));
    NMFX_HIP(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    have = bytes;
    return NMFX_OK;
}

// The HIP runtime loads a translation unit's code object onto a device lazily, at the first launch of one of its
// kernels.  So that two host threads never make those first launches at the same time, every handle passes through here
// before its own first launch: once per device, under a lock, one kernel of every translation unit is touched
// (hipFuncGetAttributes) and a launch is made and waited for.  (Precaution.  The failure that two concurrent creates did
// show -- "unknown error" on the second thread's first launch -- came from the unguarded attribute / occupancy queries of
// nmfx_phase_occupancy, which are serialised now.)
__global__ void nmfx_startup_kernel(int* p) { if (p) *p = 0; }
static int preload_once(nmfx_engine* E) {
    static std::mutex mu;
    static std::map<int, bool> done;
    std::lock_guard<std::mutex> lock(mu);
    if (done[E->device]) return NMFX_OK;
    if (nmfx_preload_bf16() || nmfx_preload_products() || nmfx_preload_mur() || nmfx_preload_kl() || nmfx_preload_phase() || nmfx_preload_aoadmm() ||
        nmfx_preload_anls() || nmfx_preload_hals() || nmfx_preload_svd() || nmfx_preload_prox() || nmfx_preload_generic() ||
        nmfx_preload_sparse()) {
        E->err = "loading the kernels onto the device failed"; return NMFX_E_HIP; }
    hipLaunchKernelGGL(nmfx_startup_kernel, dim3(1), dim3(1), 0, 0, (int*)nullptr);
    NMFX_HIP(hipGetLastError());
    NMFX_HIP(hipDeviceSynchronize());
    done[E->device] = true;
    return NMFX_OK;
}

static int64_t round_up(int64_t v, int64_t a) { return (v + a - 1) / a * a; }

__global__ void cvt_f64_rows_kernel(const double* __restrict__ src, int64_t lds, int64_t n, float* __restrict__ dst,
                                    int64_t ldd, int64_t rows)
{
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t r = blockIdx.y;
    if (c < n && r < rows) dst[r * ldd + c] = (float)src[r * lds + c];
}

__global__ void init_state_kernel(DevState* st) {
    st->flag = 0; st->stop_i = -1; st->n_obj = 0; st->obj_prev = 0.0;
    st->inner_stop = 0; st->inner_count = 0; st->notpd = 0; st->notpd_pending = 0; st->rho = 0.0; st->j_base = 0;
    st->nnls_evicted = 0; st->nnls_capped = 0; st->nnls_fallback = 0; st->nnls_noinv = 0;
    for (int i = 0; i < 4; ++i) { st->ao_hint[i >> 1][i & 1] = 0; st->ao_paths[i] = 0; }
    st->ao_continued = 0;
    for (int p = 0; p < 2; ++p) { st->pflag[p] = 0; st->pstop_i[p] = -1; st->pn_obj[p] = 0; }
    st->stop_guard = 0.0;
}

__global__ void set_guard_kernel(DevState* st, double g) { st->stop_guard = g; }
__global__ void resume_kernel(DevState* st) { st->flag = 0; st->stop_i = -1; }

__global__ void shift_iteration_base_kernel(DevState* st, long long delta) { st->j_base += delta; }

template <typename T>
static int dev_alloc(nmfx_engine* E, T** p, int64_t count) {
    NMFX_HIP(hipMalloc(reinterpret_cast<void**>(p), (size_t)count * sizeof(T)));
    NMFX_HIP(hipMemsetAsync(*p, 0, (size_t)count * sizeof(T), E->stream));
    return NMFX_OK;
}

int nmfx_ensure_obj_capacity(nmfx_engine* E, int64_t need) {
    if (need <= E->obj_cap) return NMFX_OK;
    int64_t cap = E->obj_cap ? E->obj_cap : 4096;
    while (cap < need) cap *= 2;
    double* nbuf = nullptr;
    NMFX_HIP(hipMalloc(reinterpret_cast<void**>(&nbuf), (size_t)cap * sizeof(double)));
    NMFX_HIP(hipMemsetAsync(nbuf, 0, (size_t)cap * sizeof(double), E->stream));
    if (E->obj_hist) {
        NMFX_HIP(hipMemcpyAsync(nbuf, E->obj_hist, (size_t)E->obj_cap * sizeof(double),
                                hipMemcpyDeviceToDevice, E->stream));
        NMFX_HIP(hipStreamSynchronize(E->stream));
        NMFX_HIP(hipFree(E->obj_hist));
    }
    E->obj_hist = nbuf;
    E->obj_cap = cap;
    return NMFX_OK;
}

int nmfx_ensure_inner_capacity(nmfx_engine* E, int64_t need) {
    if (need <= E->inner_cap) return NMFX_OK;
    int64_t cap = E->inner_cap ? E->inner_cap : 4096;
    while (cap < need) cap *= 2;
    int32_t* nbuf = nullptr;
    NMFX_HIP(hipMalloc(reinterpret_cast<void**>(&nbuf), (size_t)cap * 2 * sizeof(int32_t)));
    NMFX_HIP(hipMemsetAsync(nbuf, 0, (size_t)cap * 2 * sizeof(int32_t), E->stream));
    if (E->inner_hist) {
        NMFX_HIP(hipMemcpyAsync(nbuf, E->inner_hist, (size_t)E->inner_cap * 2 * sizeof(int32_t),
                                hipMemcpyDeviceToDevice, E->stream));
        NMFX_HIP(hipStreamSynchronize(E->stream));
        NMFX_HIP(hipFree(E->inner_hist));
    }
    E->inner_hist = nbuf;
    E->inner_cap = cap;
    return NMFX_OK;
}

// ---- the entry guard (nmfx_internal.h) ---------------------------
int nmfx_enter(nmfx_engine* E, const nmfx_entry& a) {
    if (!a.pre_after_bad) E->derived.drop(a.pre);
    if (!E->have_v || !E->have_f) { E->err = E->sp ? "upload the CSR matrix and set factors first" : "upload V and set factors first"; return NMFX_E_STATE; }
    if (!a.bad.empty() && !a.bad_last) { E->err = a.bad; return a.bad_rc; }
    if (a.pre_after_bad) E->derived.drop(a.pre);
    const bool pair = a.family == NMFX_FAM_MUR_PAIR;
    const int fam = pair ? NMFX_FAM_MUR : a.family;
    if (fam != NMFX_FAM_NONE) {
        if (E->run.family && E->run.family != fam) {
            E->err = "another solver has run on this handle since nmfx_set_factors: read the factors back and set them again "
                     "(nmfx_get_factors, nmfx_set_factors) before a different solver continues from them";
            return NMFX_E_STATE;
        }
        E->run.family = fam;
    }
    if (fam == NMFX_FAM_MUR) {                         // one k = 128 problem or two stacked ones: chosen at the start of the run
        if (!pair && E->run.pair) { E->err = "this handle runs two stacked problems (nmfx_mur_pair_run): nmfx_set_factors before a single-problem run"; return NMFX_E_STATE; }
        if (pair && !E->run.pair && E->run.started) { E->err = "pair mode cannot continue a run that was started as one k = 128 problem (nmfx_set_factors first)"; return NMFX_E_STATE; }
        E->run.pair = pair;
        E->run.started = true;
    }
    if (!a.bad.empty()) { E->err = a.bad; return a.bad_rc; }
    E->derived.void_all_but(a.keep);
    NMFX_HIP(hipSetDevice(E->device));
    return nmfx_ensure_obj_capacity(E, pair ? 2 * (a.first + a.count) + 8 : a.first + a.count + 2);
}

extern "C" {

int nmfx_version(void) { return 397; }      // 397: HALS on sparse handles with 129 .. 256 components (nmfx_hals_sparse_wide_run, nmfx_hals_sparse_wide_finish); 396: HALS beyond 128 components (nmfx_hals_wide_run); 395: MUR fold-in on sparse and masked handles (nmfx_sparse_foldin_run, nmfx_sparse_foldin_get_iters); 394: dense HALS fold-in (nmfx_hals_foldin_dense_run, nmfx_hals_foldin_dense_get_sweeps); 393: HALS fold-in on sparse and masked handles (nmfx_hals_foldin_run, nmfx_hals_foldin_get_sweeps); 392: HALS on masked handles (nmfx_hals_masked_run, nmfx_hals_masked_finish); 391: HALS on sparse handles (nmfx_hals_sparse_run, nmfx_hals_sparse_finish); 390: stacked HALS (nmfx_hals_stack_*); 380: HALS (nmfx_hals_run); 370: fold-in, H for new data against a fixed W (nmfx_foldin_run, nmfx_foldin_finish); 360: automatic relevance determination on the beta path (nmfx_set_ard, nmfx_clear_ard, nmfx_get_relevance); 350: NMFX_BETA, nmfx_set_beta (the beta-divergence through nmfx_mur_run / nmfx_mur_finish); 340: per-entry weights (nmfx_upload_weights, nmfx_clear_weights); 330: NMFX_IS (nmfx_mur_run / nmfx_mur_finish); 320: masked sparse handles (nmfx_set_masked); 310: sparse handles (nmfx_create_csr, nmfx_upload_csr); 300: nmfx_set_exchange_buffers takes sizes; nmfx_comm_*; k <= 256

int nmfx_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

const char* nmfx_last_error(nmfx_handle_t h) { return h ? h->err.c_str() : g_err.c_str(); }

int nmfx_create(nmfx_handle_t* out, int device, int64_t m, int64_t n, int k) {
    if (!out) { g_err = "out is NULL"; return NMFX_E_ARG; }
    *out = nullptr;
    if (m <= 0 || n <= 0 || k <= 0) { g_err = "m, n, k must be positive"; return NMFX_E_ARG; }
    if (k > 4096) { g_err = "k > 4096 is not supported"; return NMFX_E_ARG; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { g_err = "no HIP device"; return NMFX_E_HIP; }
    if (device < 0 || device >= ndev) { g_err = "device index out of range"; return NMFX_E_ARG; }
    nmfx_engine* E = new nmfx_engine();
    E->device = device; E->m = m; E->n = n; E->k = k;
    // (k > 128: a multiple of 128 -- the MUR solvers compose their iteration from the generic product kernel, kernels_generic.hip)
    E->kp = k <= 16 ? 16 : k <= 32 ? 32 : k <= 64 ? 64 : k <= 128 ? 128 : (int)round_up(k, 128);
    // 128: the split-bf16 kernel works on 128-row blocks of V and of V^T; the f32 kernels need 64
    E->mp = round_up(m, 2 * NMFX_TILE); E->np = round_up(n, 2 * NMFX_TILE);
    auto fail = [&](int rc) { g_err = E->err; nmfx_destroy(E); return rc; };
#define TRY(x) do { int rc_ = (x); if (rc_) return fail(rc_); } while (0)
#define TRYHIP(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { E->err = std::string(#x) + ": " + hipGetErrorString(e_); return fail(NMFX_E_HIP); } } while (0)
    TRYHIP(hipSetDevice(device));
    TRY(preload_once(E));
    TRYHIP(hipStreamCreateWithFlags(&E->own_stream, hipStreamNonBlocking));
    E->stream = E->own_stream;
    // split configuration: enough workgroups to fill 256 CUs twice over
    const int64_t rb = E->mp / 64, cb = E->np / 64;
    // grids = a whole number of resident rounds: 256 CUs x blocks/CU of each kernel
    int wocc = 2, hocc = 2, ncu = 256;
    nmfx_phase_occupancy(E->kp, &wocc, &hocc);
    { hipDeviceProp_t prop; if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0) ncu = prop.multiProcessorCount; }
    E->ncu = ncu;
    { const char* pm = getenv("NMFX_PRECISION");
      E->precision = (pm && (!strcmp(pm, "f32") || !strcmp(pm, "fp32"))) ? 0 : (pm && !strcmp(pm, "bf16")) ? 1 : NMFX_DEFAULT_PRECISION; }
    const char* ev;
    const int64_t wtarget = (ev = getenv("NMFX_WBLOCKS")) ? atoll(ev) : (int64_t)ncu * wocc;
    const int64_t htarget = (ev = getenv("NMFX_HBLOCKS")) ? atoll(ev) : (int64_t)ncu * hocc;
    int64_t ws = std::max<int64_t>(1, (wtarget + rb / 2) / rb); ws = std::min<int64_t>(ws, std::max<int64_t>(1, cb / 4));
    int64_t hs = std::max<int64_t>(1, (htarget + cb / 2) / cb); hs = std::min<int64_t>(hs, rb);
    int64_t gs = std::min<int64_t>(32, std::max<int64_t>(1, std::min(E->mp, E->np) / 256));   // Gram kernels: gs x kp/16 blocks
    E->wsplit = (int)ws; E->hsplit = (int)hs; E->gsplit = (int)gs;
    const int64_t kp = E->kp, mp = E->mp, np = E->np;
    TRY(dev_alloc(E, &E->V, mp * np));
    TRY(dev_alloc(E, &E->W[0], mp * kp));
    TRY(dev_alloc(E, &E->W[1], mp * kp));
    TRY(dev_alloc(E, &E->H, kp * np));
    TRY(dev_alloc(E, &E->HHt, kp * kp));
    // (the split-bf16 path spreads its Gram by-products over up to 8 row blocks x splits slabs)
    TRY(dev_alloc(E, &E->HHt_part, std::max<int64_t>(std::max(gs, ws), 40) * kp * kp));
    TRY(dev_alloc(E, &E->G_part, std::max<int64_t>(std::max(gs, hs), 4 * std::max<int64_t>(hs, (int64_t)ncu) + 8) * kp * kp));
    TRY(dev_alloc(E, &E->A_part, ws * mp * kp));
    TRY(dev_alloc(E, &E->B_part, hs * kp * np));
    E->obj_part_cap = 2 * (std::max<int64_t>(rb * ws, cb * hs) + 64) + 2 * (int64_t)ncu;      // (+ 2 ncu: the segments of a stream-K plan, at most workers + row blocks)
    TRY(dev_alloc(E, &E->obj_part, E->obj_part_cap));      // (x 2: pair mode keeps two partials per block)
    TRY(dev_alloc(E, &E->xf32, kp * np + kp * kp + kp + NMFX_XTAIL));
    TRY(dev_alloc(E, &E->xf64, 8 + 4 * NMFX_MAX_FUSED_ROUNDS));
    TRY(dev_alloc(E, &E->state, 1));
    hipLaunchKernelGGL(init_state_kernel, dim3(1), dim3(1), 0, E->stream, E->state);
    TRYHIP(hipGetLastError());
    TRY(nmfx_ensure_obj_capacity(E, 4096));
    TRYHIP(hipStreamSynchronize(E->stream));
    {   // Memory plan of the split-bf16 path: tile-major V and V^T next to the row-major V while they are built (three
        // V-sized buffers), two afterwards when the row-major one is dropped.  It is dropped for V >= 4 GiB (or
        // NMFX_DROP_V=1 / 0) and rebuilt on demand (nmfx_need_v).  If even the three-copy peak does not fit, the engine
        // runs the exact-f32 kernels (one copy) and SAYS so: nmfx_get_note().
        const double vbytes = (double)mp * (double)np * 4.0;
        const char* dv = getenv("NMFX_DROP_V");
        E->drop_v = dv ? atoi(dv) != 0 : vbytes >= 4.0 * 1024 * 1024 * 1024;
        size_t free_b = 0, total_b = 0;
        if (E->precision == 1 && nmfx_bf16_supported(E) && hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
            const double need = 2.0 * vbytes + 64.0 * (double)(mp + np) * kp + (256u << 20);
            if ((double)free_b < need) {
                E->precision = 0;
                char buf[256];
                snprintf(buf, sizeof buf, "split-bf16 products need %.1f GiB more device memory than the %.1f GiB that are free: "
                         "running the exact-f32 kernels (about half the speed)", need / 1073741824.0, (double)free_b / 1073741824.0);
                E->note = buf;
            }
        }
    }
#undef TRY
#undef TRYHIP
    *out = E;
    return NMFX_OK;
}

int nmfx_create_csr(nmfx_handle_t* out, int device, int64_t m, int64_t n, int k, int64_t nnz) {
    if (!out) { g_err = "out is NULL"; return NMFX_E_ARG; }
    *out = nullptr;
    if (m <= 0 || n <= 0 || nnz < 0) { g_err = "create_csr: m, n must be positive and nnz >= 0"; return NMFX_E_ARG; }
    if (k < 1 || k > 256) { g_err = "create_csr: sparse input supports 1 <= k <= 256 components"; return NMFX_E_ARG; }
    if (m > INT32_MAX || n > INT32_MAX || nnz > m * n) { g_err = "create_csr: m, n < 2^31 and nnz <= m n"; return NMFX_E_ARG; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { g_err = "no HIP device"; return NMFX_E_HIP; }
    if (device < 0 || device >= ndev) { g_err = "device index out of range"; return NMFX_E_ARG; }
    nmfx_engine* E = new nmfx_engine();
    E->device = device; E->m = m; E->n = n; E->k = k;
    E->kp = k <= 4 ? 4 : k <= 8 ? 8 : k <= 16 ? 16 : k <= 32 ? 32 : k <= 64 ? 64 : k <= 128 ? 128 : 256;
    E->mp = m; E->np = n;
    auto fail = [&](int rc) { g_err = E->err; nmfx_destroy(E); return rc; };
    if (hipSetDevice(device) != hipSuccess) { E->err = "hipSetDevice failed"; return fail(NMFX_E_HIP); }
    int rc;
    if ((rc = preload_once(E))) return fail(rc);
    if (hipStreamCreateWithFlags(&E->own_stream, hipStreamNonBlocking) != hipSuccess) { E->err = "hipStreamCreate failed"; return fail(NMFX_E_HIP); }
    E->stream = E->own_stream;
    { hipDeviceProp_t prop; if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0) E->ncu = prop.multiProcessorCount; }
    E->precision = 0;
    if ((rc = dev_alloc(E, &E->xf64, 8))) return fail(rc);
    if ((rc = dev_alloc(E, &E->state, 1))) return fail(rc);
    hipLaunchKernelGGL(init_state_kernel, dim3(1), dim3(1), 0, E->stream, E->state);
    if (hipGetLastError() != hipSuccess) { E->err = "init_state launch failed"; return fail(NMFX_E_HIP); }
    if ((rc = nmfx_ensure_obj_capacity(E, 4096))) return fail(rc);
    if ((rc = nmfx_sparse_init(E, nnz))) return fail(rc);
    *out = E;
    return NMFX_OK;
}

int nmfx_destroy(nmfx_handle_t E) {
    if (!E) return NMFX_OK;
    hipSetDevice(E->device);
    if (E->stream) hipStreamSynchronize(E->stream);
    nmfx_sparse_free(E);
    nmfx_comm_free(E);
    for (auto& t : E->prof_pending) { hipEventDestroy(std::get<1>(t)); hipEventDestroy(std::get<2>(t)); }
    void* bufs[] = {E->V, E->W[0], E->W[1], E->H, E->HHt, E->HHt_part, E->G_part, E->A_part, E->B_part,
                    E->obj_part, E->phase_part, E->Om, E->ard_sums, E->ard_lam, E->ard_pen, E->own_x ? (void*)E->xf32 : nullptr, E->own_x ? (void*)E->xf64 : nullptr,
                    E->obj_hist, E->state, E->dualW, E->dualH, E->auxW, E->auxH, E->Minv, E->nrm_part,
                    E->inner_hist, E->Pw, E->Ph, E->Asum, E->S, E->DV, E->Vt, E->Vtile, E->Bt_part, E->Whi[0], E->Whi[1],
                    E->Wlo[0], E->Wlo[1], E->WThi, E->WTlo, E->Hhi, E->Hlo, E->HThi, E->HTlo, E->nrm_rounds, E->bkX, E->bkU,
                    E->nnls_ginv, E->nnls_todo, E->G_big, E->kl_part, E->Bt_chunk, E->gx_part, E->gx_d, E->gx_s, E->gx_r, E->gx_w64, E->gx_nrm, E->prox_keys, E->gx_nnls_work,
                    E->gxb_v[0], E->gxb_v[1], E->gxb_v[2], E->gxb_v[3], E->gxb_vt, E->gxb_q[0], E->gxb_q[1],
                    E->kl_S[0], E->kl_S[1], E->kl_DV[0], E->kl_DV[1], E->sk[0].seg, E->sk[0].first, E->sk[0].cnt, E->sk[0].slabs, E->sk[1].seg, E->sk[1].first, E->sk[1].cnt, E->sk[1].slabs, E->minv_img, E->gx_gimg,
                    E->stack_dev, E->stack_obj, E->stack_part, E->foldin_dense_sweeps};
    for (void* b : bufs) if (b) hipFree(b);
    if (E->own_stream) hipStreamDestroy(E->own_stream);
    delete E;
    return NMFX_OK;
}

int nmfx_set_stream(nmfx_handle_t E, void* s) {
    if (!E) return NMFX_E_ARG;
    NMFX_HIP(hipSetDevice(E->device));
    NMFX_HIP(hipStreamSynchronize(E->stream));
    E->stream = reinterpret_cast<hipStream_t>(s);      // NULL = HIP's default (null) stream
    return NMFX_OK;
}

int nmfx_reset_stream(nmfx_handle_t E) {
    if (!E) return NMFX_E_ARG;
    NMFX_HIP(hipSetDevice(E->device));
    NMFX_HIP(hipStreamSynchronize(E->stream));
    E->stream = E->own_stream;
    return NMFX_OK;
}

int nmfx_set_precision(nmfx_handle_t E, int mode) {
    NMFX_NOT_SPARSE(E);
    if (!E || (mode != 0 && mode != 1)) { if (E) E->err = "precision must be 0 (f32) or 1 (split bf16)"; return NMFX_E_ARG; }
    // kept: what does not consist of bf16 images of the factors (the KL leftovers are tied to their iteration index instead)
    E->derived.void_all_but(NMFX_D_kl_h_iter | NMFX_D_lazy_objective | NMFX_D_anls_a_ready | NMFX_D_kl_bt_ready | NMFX_D_ard_valid);
    if (E->precision != mode) nmfx_comm_invalidate(E);
    E->precision = mode;
    return NMFX_OK;
}

const char* nmfx_get_note(nmfx_handle_t E) { return E ? E->note.c_str() : ""; }

int nmfx_get_precision(nmfx_handle_t E) {
    NMFX_NOT_SPARSE(E);
    if (!E) return NMFX_E_ARG;
    return (E->precision == 1 && nmfx_bf16_supported(E)) ? 1 : 0;
}

int nmfx_synchronize(nmfx_handle_t E) {
    if (!E) return NMFX_E_ARG;
    NMFX_HIP(hipSetDevice(E->device));
    NMFX_HIP(hipStreamSynchronize(E->stream));
    return NMFX_OK;
}

// f64 rows in device memory (row stride lds) -> f32 rows of a padded [..][np] device matrix.  One row per grid.y entry: at
// most CVT_MAX_ROWS rows per launch (grid.y ends at 65535), every launch checked.  Both upload paths convert through here.
static const int64_t CVT_MAX_ROWS = 32768;
static hipError_t cvt_f64_rows(nmfx_engine* E, const double* src, int64_t lds, float* dst, int64_t rows) {
    for (int64_t r = 0; r < rows; r += CVT_MAX_ROWS) {
        const int64_t cnt = std::min<int64_t>(CVT_MAX_ROWS, rows - r);
        dim3 grid((unsigned)((E->n + 255) / 256), (unsigned)cnt);
        hipLaunchKernelGGL(cvt_f64_rows_kernel, grid, dim3(256), 0, E->stream, src + r * lds, lds, E->n,
                           dst + r * E->np, E->np, cnt);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// rows of a host matrix (row stride ld, dtype NMFX_F32 / NMFX_F64) into rows of a padded [..][np] f32 device matrix
static int copy_rows_in(nmfx_engine* E, float* dst, const void* host, int dtype, int64_t ld, int64_t rows, const char* who) {
    if (dtype == NMFX_F32) {
        NMFX_HIP(hipMemcpy2DAsync(dst, (size_t)E->np * 4, host, (size_t)ld * 4, (size_t)E->n * 4,
                                  (size_t)rows, hipMemcpyHostToDevice, E->stream));
        NMFX_HIP(hipStreamSynchronize(E->stream));
    } else if (dtype == NMFX_F64) {
        const int64_t chunk = std::max<int64_t>(1, (int64_t)(64 << 20) / (E->n * 8));
        double* stage = nullptr;
        NMFX_HIP(hipMalloc(reinterpret_cast<void**>(&stage), (size_t)std::min(chunk, rows) * E->n * 8));
        const double* src = static_cast<const double*>(host);
        for (int64_t r = 0; r < rows; r += chunk) {
            const int64_t cnt = std::min(chunk, rows - r);
            hipError_t e = hipMemcpy2DAsync(stage, (size_t)E->n * 8, src + r * ld, (size_t)ld * 8,
                                            (size_t)E->n * 8, (size_t)cnt, hipMemcpyHostToDevice, E->stream);
            if (e == hipSuccess) e = cvt_f64_rows(E, stage, E->n, dst + r * E->np, cnt);
            if (e == hipSuccess) e = hipStreamSynchronize(E->stream);
            if (e != hipSuccess) { hipFree(stage); E->err = std::string(who) + ": " + hipGetErrorString(e); return NMFX_E_HIP; }
        }
        hipFree(stage);
    } else { E->err = std::string(who) + ": dtype must be NMFX_F32 or NMFX_F64"; return NMFX_E_ARG; }
    return NMFX_OK;
}

int nmfx_upload_v(nmfx_handle_t E, const void* host, int dtype, int64_t ld, int64_t row0, int64_t rows) {
    NMFX_NOT_SPARSE(E);
    if (!E) return NMFX_E_ARG;
    if (!host || row0 < 0 || rows < 0 || row0 + rows > E->m || ld < E->n) {
        E->err = "upload_v: bad row range or leading dimension"; return NMFX_E_ARG; }
    if (dtype != NMFX_F32 && dtype != NMFX_F64) { E->err = "upload_v: dtype must be NMFX_F32 or NMFX_F64"; return NMFX_E_ARG; }
    E->derived.drop(NMFX_D_anls_a_ready);              // (products with V)
    NMFX_HIP(hipSetDevice(E->device));
    if (rows == 0) return NMFX_OK;
    if (E->have_v) { int rc_ = nmfx_need_v(E); if (rc_) return rc_; }       // (rows of a V whose row-major copy was dropped)
    { int rc_ = copy_rows_in(E, E->V + row0 * E->np, host, dtype, ld, rows, "upload_v"); if (rc_) return rc_; }
    E->have_v = true;
    E->stack_vv_ready = false;
    E->bf_ready = false;
    E->gxb_v_ready = false;
    E->gxb_vt_ready = false;
    return NMFX_OK;
}

// Per-entry weights (version 340): a second [mp][np] f32 matrix beside V, zero where nothing was uploaded (padding included).
static const char* const WEIGHTS_NOTE = "per-entry weights are present: MUR runs the weighted exact-f32 kernels whatever the precision mode";
int nmfx_upload_weights(nmfx_handle_t E, const void* host, int dtype, int64_t ld, int64_t row0, int64_t rows) {
    if (!E) return NMFX_E_ARG;
    if (E->sp) { E->err = "upload_weights: not available on a sparse handle (its stored entries are its 0 / 1 weights: nmfx_set_masked)"; return NMFX_E_ARG; }
    if (E->kp > 128) { E->err = "upload_weights: per-entry weights need k <= 128"; return NMFX_E_ARG; }
    if (!host || row0 < 0 || rows < 0 || row0 + rows > E->m || ld < E->n) {
        E->err = "upload_weights: bad row range or leading dimension"; return NMFX_E_ARG; }
    if (dtype != NMFX_F32 && dtype != NMFX_F64) { E->err = "upload_weights: dtype must be NMFX_F32 or NMFX_F64"; return NMFX_E_ARG; }
    NMFX_HIP(hipSetDevice(E->device));
    if (!E->Om) {
        const size_t bytes = (size_t)E->mp * E->np * sizeof(float);
        float* buf = nullptr;
        if (hipMalloc(reinterpret_cast<void**>(&buf), bytes) != hipSuccess) {
            (void)hipGetLastError();
            E->err = "upload_weights: the weights (" + std::to_string(bytes >> 20) + " MiB, the size of V) do not fit into the free device memory";
            return NMFX_E_NOMEM;
        }
        hipError_t e = hipMemsetAsync(buf, 0, bytes, E->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(E->stream);
        if (e != hipSuccess) { hipFree(buf); E->err = hipGetErrorString(e); return NMFX_E_HIP; }
        E->Om = buf;
        if (E->note.find(WEIGHTS_NOTE) == std::string::npos) E->note += (E->note.empty() ? "" : "; ") + std::string(WEIGHTS_NOTE);
    }
    E->derived.drop(NMFX_D_anls_a_ready);
    if (rows == 0) return NMFX_OK;
    return copy_rows_in(E, E->Om + row0 * E->np, host, dtype, ld, rows, "upload_weights");
}

int nmfx_clear_weights(nmfx_handle_t E) {
    if (!E) return NMFX_E_ARG;
    if (!E->Om) return NMFX_OK;
    NMFX_HIP(hipSetDevice(E->device));
    NMFX_HIP(hipStreamSynchronize(E->stream));
    NMFX_HIP(hipFree(E->Om));
    E->Om = nullptr;
    E->derived.drop(NMFX_D_anls_a_ready);
    const std::string w(WEIGHTS_NOTE);
    size_t at = E->note.find(w);
    if (at != std::string::npos) {
        size_t len = w.size();
        if (at >= 2 && E->note.compare(at - 2, 2, "; ") == 0) { at -= 2; len += 2; }
        else if (E->note.compare(at + len, 2, "; ") == 0) len += 2;
        E->note.erase(at, len);
    }
    return NMFX_OK;
}

// The beta of NMFX_BETA runs (version 350).  The range is what f32 carries: q = 1e-9 in a real cell, q^(beta - 2) v finite.
int nmfx_set_beta(nmfx_handle_t E, double beta) {
    if (!E) return NMFX_E_ARG;
    if (E->sp) { E->err = "set_beta: the beta-divergence is not available on a sparse handle (dense V, k <= 128)"; return NMFX_E_ARG; }
    if (E->kp > 128) { E->err = "set_beta: the beta-divergence needs k <= 128"; return NMFX_E_ARG; }
    if (!(beta >= -1.0 && beta <= 3.0)) { E->err = "set_beta: beta must lie in [-1, 3] (what f32 carries at q = 1e-9)"; return NMFX_E_ARG; }
    E->beta = beta;
    E->beta_set = true;
    E->derived.drop(NMFX_D_ard_valid);                 // (ARD stays set; its relevances are recomputed before the next run)
    static const char* const BETA_NOTE = "the beta-divergence (NMFX_BETA) runs the exact-f32 kernels; the split-bf16 mode does not apply to it";
    if (E->note.find(BETA_NOTE) == std::string::npos) E->note += (E->note.empty() ? "" : "; ") + std::string(BETA_NOTE);
    return NMFX_OK;
}

// Automatic relevance determination on the beta path (version 360; kernels_phase.hip)
int nmfx_set_ard(nmfx_handle_t E, double phi, double a, double b) {
    if (!E) return NMFX_E_ARG;
    if (E->sp) { E->err = "set_ard: automatic relevance determination is not available on a sparse handle (dense V, k <= 128)"; return NMFX_E_ARG; }
    if (E->kp > 128) { E->err = "set_ard: automatic relevance determination needs k <= 128"; return NMFX_E_ARG; }
    if (!(std::isfinite(phi) && phi > 0.0 && std::isfinite(a) && a > 0.0 && std::isfinite(b) && b > 0.0)) {
        E->err = "set_ard: phi, a and b must be finite and > 0"; return NMFX_E_ARG; }
    if (!E->beta_set) { E->err = "set_ard: no beta set (nmfx_set_beta): automatic relevance determination runs on the beta-divergence"; return NMFX_E_STATE; }
    NMFX_HIP(hipSetDevice(E->device));
    { int rc_ = nmfx_ard_alloc(E); if (rc_) return rc_; }
    E->ard_phi = phi; E->ard_a = a; E->ard_b = b;
    E->ard = true;
    E->derived.drop(NMFX_D_ard_valid);
    return NMFX_OK;
}

int nmfx_clear_ard(nmfx_handle_t E) {
    if (!E) return NMFX_E_ARG;
    E->ard = false;
    E->derived.drop(NMFX_D_ard_valid);
    return NMFX_OK;
}

// the relevances of (W, H) where they are not the current ones: at the start of a run, after nmfx_set_beta / nmfx_set_ard
static int ard_ensure(nmfx_engine* E, const float* W) {
    if (!E->ard || E->derived.ard_valid) return NMFX_OK;
    int rc = nmfx_ard_relevance(E, W, false);
    if (!rc) E->derived.ard_valid = true;
    return rc;
}

static int read_state(nmfx_engine* E, DevState* hs);
int nmfx_get_relevance(nmfx_handle_t E, double* lambda_out) {
    if (!E || !lambda_out) { if (E) E->err = "get_relevance: lambda_out is NULL"; return NMFX_E_ARG; }
    if (!E->ard) { E->err = "get_relevance: automatic relevance determination is not set (nmfx_set_ard)"; return NMFX_E_STATE; }
    if (!E->have_f) { E->err = "get_relevance: set factors first"; return NMFX_E_STATE; }
    DevState hs; int rc;
    if ((rc = read_state(E, &hs))) return rc;
    if (hs.flag && !E->run.w_in_place) E->run.wsel = (int)((hs.stop_i + 1) & 1);
    if ((rc = ard_ensure(E, E->W[E->run.wsel]))) return rc;
    NMFX_HIP(hipMemcpyAsync(lambda_out, E->ard_lam, (size_t)E->k * sizeof(double), hipMemcpyDeviceToHost, E->stream));
    NMFX_HIP(hipStreamSynchronize(E->stream));
    return NMFX_OK;
}

int nmfx_upload_v_device(nmfx_handle_t E, const void* dev, int dtype, int64_t ld, int64_t row0, int64_t rows) {
    NMFX_NOT_SPARSE(E);
    if (!E) return NMFX_E_ARG;
    if (!dev || row0 < 0 || rows < 0 || row0 + rows > E->m || ld < E->n) {
        E->err = "upload_v_device: bad row range or leading dimension"; return NMFX_E_ARG; }
    if (dtype != NMFX_F32 && dtype != NMFX_F64) { E->err = "upload_v_device: dtype must be NMFX_F32 or NMFX_F64"; return NMFX_E_ARG; }
    E->derived.drop(NMFX_D_anls_a_ready);
    NMFX_HIP(hipSetDevice(E->device));
    if (rows == 0) return NMFX_OK;
    if (E->have_v) { int rc_ = nmfx_need_v(E); if (rc_) return rc_; }
    float* dst = E->V + row0 * E->np;
    if (dtype == NMFX_F32) {
        NMFX_HIP(hipMemcpy2DAsync(dst, (size_t)E->np * 4, dev, (size_t)ld * 4, (size_t)E->n * 4,
                                  (size_t)rows, hipMemcpyDeviceToDevice, E->stream));
    } else if (dtype == NMFX_F64) {
        NMFX_HIP(cvt_f64_rows(E, static_cast<const double*>(dev), ld, dst, rows));
    } else { E->err = "upload_v_device: dtype must be NMFX_F32 or NMFX_F64"; return NMFX_E_ARG; }
    NMFX_HIP(hipStreamSynchronize(E->stream));
    E->have_v = true;
    E->stack_vv_ready = false;
    E->bf_ready = false;
    E->gxb_v_ready = false;
    E->gxb_vt_ready = false;
    return NMFX_OK;
}

static int put_padded(nmfx_engine* E, float* dst, const double* src, int64_t rows, int64_t cols,
                      int64_t prow, int64_t pcol) {
    std::vector<float> tmp((size_t)prow * pcol, 0.f);
    for (int64_t r = 0; r < rows; ++r)
        for (int64_t c = 0; c < cols; ++c) tmp[(size_t)r * pcol + c] = (float)src[r * cols + c];
    NMFX_HIP(hipMemcpyAsync(dst, tmp.data(), tmp.size() * 4, hipMemcpyHostToDevice, E->stream));
    NMFX_HIP(hipStreamSynchronize(E->stream));
    return NMFX_OK;
}

static int get_padded(nmfx_engine* E, const float* src, double* dst, int64_t rows, int64_t cols,
                      int64_t prow, int64_t pcol) {
    std::vector<float> tmp((size_t)prow * pcol);
    NMFX_HIP(hipMemcpyAsync(tmp.data(), src, tmp.size() * 4, hipMemcpyDeviceToHost, E->stream));
    NMFX_HIP(hipStreamSynchronize(E->stream));
    for (int64_t r = 0; r < rows; ++r)
        for (int64_t c = 0; c < cols; ++c) dst[r * cols + c] = (double)tmp[(size_t)r * pcol + c];
    return NMFX_OK;
}

int nmfx_set_factors(nmfx_handle_t E, const double* w, const double* hmat) {
    if (!E) return NMFX_E_ARG;
    if (E->sp) {                                       // (the same reset of the iteration state as below, then the sparse layouts)
        NMFX_HIP(hipSetDevice(E->device));
        hipLaunchKernelGGL(init_state_kernel, dim3(1), dim3(1), 0, E->stream, E->state);
        NMFX_HIP(hipGetLastError());
        return nmfx_sparse_set_factors(E, w, hmat);
    }
    NMFX_HIP(hipSetDevice(E->device));
    int rc;
    if (w) {
        if ((rc = put_padded(E, E->W[0], w, E->m, E->k, E->mp, E->kp))) return rc;
        NMFX_HIP(hipMemsetAsync(E->W[1], 0, (size_t)E->mp * E->kp * 4, E->stream));
    }
    if (hmat) { if ((rc = put_padded(E, E->H, hmat, E->k, E->n, E->kp, E->np))) return rc; }
    // (S, DV: the m x n auxiliaries of the KL-loss ADMM variants start from zero, ao_admm.py:17-30)
    float* zero[] = {E->dualW, E->dualH, E->auxW, E->auxH, E->S, E->DV, E->kl_S[0], E->kl_DV[0], E->kl_S[1], E->kl_DV[1]};
    const int64_t mn = E->mp * E->np;
    const int64_t zc[] = {E->mp * E->kp, E->kp * E->np, E->mp * E->kp, E->kp * E->np, mn, mn, mn, mn, mn, mn};
    E->kl_side = 0; E->kl_s_side = 0;                  // (split-bf16 form of the same state: zero in both orientations)
    for (int i = 0; i < 10; ++i)
        if (zero[i]) NMFX_HIP(hipMemsetAsync(zero[i], 0, (size_t)zc[i] * 4, E->stream));
    hipLaunchKernelGGL(init_state_kernel, dim3(1), dim3(1), 0, E->stream, E->state);
    if ((rc = nmfx_hals_stack_reset(E))) return rc;
    E->have_f = true;
    E->bf_ready = false;
    E->derived.void_all_but(NMFX_D_NONE);
    E->run.reset();
    if (E->kp <= 128 && (rc = nmfx_launch_gram_nt(E, E->H, E->np, E->np, E->HHt_part, E->gsplit))) return rc;
    NMFX_HIP(hipStreamSynchronize(E->stream));
    return NMFX_OK;
}

static int read_state(nmfx_engine* E, DevState* hs) {
    NMFX_HIP(hipSetDevice(E->device));
    NMFX_HIP(hipMemcpyAsync(hs, E->state, sizeof(DevState), hipMemcpyDeviceToHost, E->stream));
    NMFX_HIP(hipStreamSynchronize(E->stream));
    return NMFX_OK;
}

int nmfx_get_factors(nmfx_handle_t E, double* w, double* hmat) {
    if (!E) return NMFX_E_ARG;
    if (E->sp) return nmfx_sparse_get_factors(E, w, hmat);
    DevState hs; int rc;
    if ((rc = read_state(E, &hs))) return rc;
    if (hs.flag && !E->run.w_in_place) E->run.wsel = (int)((hs.stop_i + 1) & 1);
    if (w) { if ((rc = get_padded(E, E->W[E->run.wsel], w, E->m, E->k, E->mp, E->kp))) return rc; }
    if (hmat) { if ((rc = get_padded(E, E->H, hmat, E->k, E->n, E->kp, E->np))) return rc; }
    return NMFX_OK;
}

int nmfx_get_matrix(nmfx_handle_t E, const char* name, double* out) {
    NMFX_NOT_SPARSE(E);
    if (!E || !name || !out) return NMFX_E_ARG;
    NMFX_HIP(hipSetDevice(E->device));
    const std::string s(name);
    const float* src = nullptr; bool wlike = false;
    if (s == "dual_w") { src = E->dualW; wlike = true; }
    else if (s == "dual_h") { src = E->dualH; }
    else if (s == "w_aux") { src = E->auxW; wlike = true; }
    else if (s == "h_aux") { src = E->auxH; }
    else { E->err = "get_matrix: unknown name"; return NMFX_E_ARG; }
    if (!src) { E->err = "get_matrix: matrix not allocated for this solver"; return NMFX_E_STATE; }
    return wlike ? get_padded(E, src, out, E->m, E->k, E->mp, E->kp)
                 : get_padded(E, src, out, E->k, E->n, E->kp, E->np);
}

int nmfx_set_matrix(nmfx_handle_t E, const char* name, const double* in) {
    NMFX_NOT_SPARSE(E);
    if (!E || !name || !in) return NMFX_E_ARG;
    NMFX_HIP(hipSetDevice(E->device));
    int rc;
    if ((rc = nmfx_admm_state_alloc(E))) return rc;
    const std::string s(name);
    float* dst = nullptr; bool wlike = false;
    if (s == "dual_w") { dst = E->dualW; wlike = true; }
    else if (s == "dual_h") { dst = E->dualH; }
    else if (s == "w_aux") { dst = E->auxW; wlike = true; }
    else if (s == "h_aux") { dst = E->auxH; }
    else { E->err = "set_matrix: unknown name"; return NMFX_E_ARG; }
    return wlike ? put_padded(E, dst, in, E->m, E->k, E->mp, E->kp) : put_padded(E, dst, in, E->k, E->n, E->kp, E->np);
}

int nmfx_get_state(nmfx_handle_t E, int* stop_rule, int64_t* stop_i, int64_t* n_obj) {
    if (!E) return NMFX_E_ARG;
    DevState hs; int rc;
    if ((rc = read_state(E, &hs))) return rc;
    if (hs.notpd) { E->err = "Gram + rho I is not positive definite"; return NMFX_E_NOTPD; }
    if (stop_rule) *stop_rule = hs.flag;
    if (stop_i) *stop_i = hs.stop_i;
    if (n_obj) *n_obj = hs.n_obj;
    // the iterate the reference would return: W_{stop_i+1} once stopped
    if (hs.flag && !E->run.w_in_place) E->run.wsel = (int)((hs.stop_i + 1) & 1);
    return NMFX_OK;
}

int nmfx_get_diagnostics(nmfx_handle_t E, int64_t* nnls_evicted, int64_t* nnls_capped) {
    NMFX_NOT_SPARSE(E);
    if (!E) return NMFX_E_ARG;
    DevState hs; int rc;
    if ((rc = read_state(E, &hs))) return rc;
    if (nnls_evicted) *nnls_evicted = hs.nnls_evicted;
    if (nnls_capped) *nnls_capped = hs.nnls_capped;
    return NMFX_OK;
}

int nmfx_get_nnls_fallbacks(nmfx_handle_t E, int64_t* problems, int64_t* half_steps) {
    NMFX_NOT_SPARSE(E);
    if (!E) return NMFX_E_ARG;
    DevState hs; int rc;
    if ((rc = read_state(E, &hs))) return rc;
    if (problems) *problems = hs.nnls_fallback;
    if (half_steps) *half_steps = hs.nnls_noinv;
    return NMFX_OK;
}

int nmfx_get_inner_paths(nmfx_handle_t E, int64_t out[4]) {
    NMFX_NOT_SPARSE(E);
    if (!E || !out) return NMFX_E_ARG;
    DevState hs; int rc;
    if ((rc = read_state(E, &hs))) return rc;
    for (int i = 0; i < 4; ++i) out[i] = hs.ao_paths[i];
    return NMFX_OK;
}

int nmfx_get_objectives(nmfx_handle_t E, int64_t first, int64_t count, double* out) {
    if (!E || !out || first < 0 || count < 0 || first + count > E->obj_cap) {
        if (E) E->err = "get_objectives: range"; return NMFX_E_ARG; }
    NMFX_HIP(hipSetDevice(E->device));
    if (count == 0) return NMFX_OK;
    NMFX_HIP(hipMemcpyAsync(out, E->obj_hist + first, (size_t)count * 8, hipMemcpyDeviceToHost, E->stream));
    NMFX_HIP(hipStreamSynchronize(E->stream));
    return NMFX_OK;
}

int nmfx_get_inner_counts(nmfx_handle_t E, int64_t first, int64_t count, int32_t* out) {
    NMFX_NOT_SPARSE(E);
    if (!E || !out || first < 0 || count < 0 || first + count > E->inner_cap) {
        if (E) E->err = "get_inner_counts: range"; return NMFX_E_ARG; }
    NMFX_HIP(hipSetDevice(E->device));
    if (count == 0) return NMFX_OK;
    NMFX_HIP(hipMemcpyAsync(out, E->inner_hist + first * 2, (size_t)count * 8, hipMemcpyDeviceToHost, E->stream));
    NMFX_HIP(hipStreamSynchronize(E->stream));
    return NMFX_OK;
}

// ---- exchange buffers ----------------------------------------------------
int nmfx_exchange_sizes(nmfx_handle_t E, int64_t* n_f32, int64_t* n_f64) {
    NMFX_NOT_SPARSE(E);
    if (!E) return NMFX_E_ARG;
    if (n_f32) *n_f32 = (int64_t)E->kp * E->np + (int64_t)E->kp * E->kp + E->kp + NMFX_XTAIL;
    if (n_f64) *n_f64 = 8 + 4 * NMFX_MAX_FUSED_ROUNDS;
    return NMFX_OK;
}

int nmfx_set_exchange_rank(nmfx_handle_t E, int rank, int world) {
    NMFX_NOT_SPARSE(E);
    if (!E) return NMFX_E_ARG;
    if (world == 0) { E->xrank = -1; E->xworld = 0; return NMFX_OK; }           // back to the separate f64 exchange
    if (world < 1 || world > NMFX_XTAIL_RANKS || rank < 0 || rank >= world) { E->err = "set_exchange_rank: 1 <= world <= 64, 0 <= rank < world"; return NMFX_E_ARG; }
    if (!(E->precision == 1 && nmfx_bf16_supported(E))) { E->err = "set_exchange_rank: only with the split-bf16 epilogues (k padded to 64 / 128)"; return NMFX_E_STATE; }
    E->xrank = rank; E->xworld = world;
    return NMFX_OK;
}

int nmfx_set_exchange_buffers(nmfx_handle_t E, void* f32, int64_t n_f32, void* f64, int64_t n_f64) {
    NMFX_NOT_SPARSE(E);
    if (!E || !f32 || !f64) return NMFX_E_ARG;
    int64_t need32, need64;
    nmfx_exchange_sizes(E, &need32, &need64);
    if (n_f32 < need32 || n_f64 < need64) {
        E->err = "set_exchange_buffers: allocations smaller than nmfx_exchange_sizes (the buffers grew in round 2: f64 tail of 4 x 64 "
                 "norm sums, f32 tail of 256 floats)";
        return NMFX_E_ARG;
    }
    NMFX_HIP(hipSetDevice(E->device));
    NMFX_HIP(hipStreamSynchronize(E->stream));
    if (E->own_x) { hipFree(E->xf32); hipFree(E->xf64); }
    E->xf32 = static_cast<float*>(f32); E->xf64 = static_cast<double*>(f64); E->own_x = false;
    return NMFX_OK;
}

int nmfx_get_exchange_buffers(nmfx_handle_t E, void** f32, void** f64) {
    NMFX_NOT_SPARSE(E);
    if (!E) return NMFX_E_ARG;
    if (f32) *f32 = E->xf32;
    if (f64) *f64 = E->xf64;
    return NMFX_OK;
}

// ---- the f64 referee of the stop rule (kernels_generic.hip: nmfx_objective_f64) ---------------
int nmfx_set_stop_guard(nmfx_handle_t E, double guard) {
    if (!E || !(guard >= 0.0)) { if (E) E->err = "set_stop_guard: guard >= 0"; return NMFX_E_ARG; }
    NMFX_HIP(hipSetDevice(E->device));
    hipLaunchKernelGGL(set_guard_kernel, dim3(1), dim3(1), 0, E->stream, E->state, guard);
    NMFX_HIP(hipGetLastError());
    return NMFX_OK;
}

int nmfx_resume(nmfx_handle_t E) {
    if (!E) return NMFX_E_ARG;
    NMFX_HIP(hipSetDevice(E->device));
    hipLaunchKernelGGL(resume_kernel, dim3(1), dim3(1), 0, E->stream, E->state);
    NMFX_HIP(hipGetLastError());
    return NMFX_OK;
}

// ---- iteration base (hipGraph replay support) --------------------------------
int nmfx_reserve_objectives(nmfx_handle_t E, int64_t count) {
    NMFX_NOT_SPARSE(E);
    if (!E || count < 0) return NMFX_E_ARG;
    NMFX_HIP(hipSetDevice(E->device));
    return nmfx_ensure_obj_capacity(E, count + 2);
}

int nmfx_shift_iteration_base(nmfx_handle_t E, int64_t delta) {
    NMFX_NOT_SPARSE(E);
    if (!E) return NMFX_E_ARG;
    NMFX_HIP(hipSetDevice(E->device));
    hipLaunchKernelGGL(shift_iteration_base_kernel, dim3(1), dim3(1), 0, E->stream, E->state, (long long)delta);
    NMFX_HIP(hipGetLastError());
    return NMFX_OK;
}

// ---- MUR -------------------------------------------------------------------
// What a MUR entry point keeps.  An iteration of the loss `distance`: the images of the k > 128 loop, and for KL the leftovers of
// the H epilogue (the H images and row-sum partials of iteration j are good for the KL W phase of iteration j + 1 only if NOTHING
// else has written H or those buffers in between: every other loss and every other solver voids them).  A closing step
// changes no factor and keeps both; nmfx_mur_finish_b, which closes the runs of EVERY row-sharded solver, keeps all but the
// ANLS products (its reduce goes through A_part's neighbours); the dense phase path keeps the relevances instead.
static unsigned mur_keep(int distance) { return NMFX_D_gxb_img_ready | (distance == NMFX_KL ? NMFX_D_kl_h_iter : NMFX_D_NONE); }
static const unsigned MUR_KEEP_CLOSING = NMFX_D_gxb_img_ready | NMFX_D_kl_h_iter;
static const unsigned KEEP_FINISH_B = NMFX_D_ALL & ~NMFX_D_anls_a_ready;
// (pre: a run-level or closing entry point has only ever voided the ANLS products before it asked; a phase voids all it does not keep)
static int mur_enter(nmfx_engine* E, int64_t first, int64_t count, unsigned keep, int family = NMFX_FAM_MUR, unsigned pre = NMFX_D_anls_a_ready) {
    nmfx_entry a = {family, first, count, keep, pre};
    if (first < 0 || count < 0) { a.bad = "negative iteration range"; a.bad_last = true; }
    return nmfx_enter(E, a);
}

// The Itakura-Saito divergence (NMFX_IS) runs through nmfx_mur_run / nmfx_mur_finish only (dense k <= 128, masked sparse)
static int refuse_is(nmfx_engine* E, const char* who) {
    E->err = std::string(who) + ": the Itakura-Saito divergence (IS) is available through nmfx_mur_run / nmfx_mur_finish only";
    return NMFX_E_ARG;
}
// ... and so does the beta-divergence (NMFX_BETA, nmfx_set_beta; dense k <= 128)
static int refuse_beta(nmfx_engine* E, const char* who) {
    E->err = std::string(who) + ": the beta-divergence (NMFX_BETA) is available through nmfx_mur_run / nmfx_mur_finish only";
    return NMFX_E_ARG;
}
#define NMFX_EU_KL_ONLY(E, distance) do { if ((E) && (distance) == NMFX_IS) return refuse_is((E), __func__); \
                                          if ((E) && (distance) == NMFX_BETA) return refuse_beta((E), __func__); } while (0)
// First statements of every phase-level MUR entry point (a macro: the refusals name the entry point)
#define NMFX_MUR_PHASE_ENTRY(E, distance) do { NMFX_DENSE_ONLY(E); NMFX_EU_KL_ONLY(E, distance); if (!(E)) return NMFX_E_ARG; } while (0)
// ... and what follows them where the call is one step of iteration j of a Euclidean / KL run (the f64 referee applies again)
static int mur_phase_enter(nmfx_engine* E, int64_t j, unsigned keep) {
    E->run.mur_loss(NMFX_EU);
    return mur_enter(E, j, 1, keep, NMFX_FAM_MUR, (NMFX_D_kl_h_iter | NMFX_D_himg_both | NMFX_D_anls_a_ready) & ~keep);
}
static bool mur_bf16(const nmfx_engine* E) { return E->precision == 1 && nmfx_bf16_supported(E); }

int nmfx_mur_phase_a(nmfx_handle_t E, int distance, double lambda_w, int64_t j) {
    NMFX_MUR_PHASE_ENTRY(E, distance);
    int rc = mur_phase_enter(E, j, mur_keep(distance)); if (rc) return rc;
    if (E->kp > 128 && (distance == NMFX_EU || distance == NMFX_KL)) return nmfx_generic_mur_phase_a(E, distance, lambda_w, j);
    if (distance == NMFX_EU) return mur_bf16(E) ? nmfx_mur_eu_phase_a_bf16(E, lambda_w, j) : nmfx_mur_eu_phase_a(E, lambda_w, j);
    if (distance == NMFX_KL) return mur_bf16(E) ? nmfx_mur_kl_phase_a_bf16(E, lambda_w, j) : nmfx_mur_kl_phase_a(E, lambda_w, j);
    E->err = "Unknown distance type."; return NMFX_E_ARG;
}

// Phase A in pieces (chunked exchange; Euclidean loss on the split-bf16 path only -- nmfx_mur_chunk_info says whether)
static bool mur_chunkable(nmfx_engine* E, int distance) { return distance == NMFX_EU && mur_bf16(E); }
int nmfx_mur_chunk_info(nmfx_handle_t E, int distance, int64_t* unit, int64_t* n_padded, int64_t* k_padded) {
    NMFX_MUR_PHASE_ENTRY(E, distance);
    const bool ok = mur_chunkable(E, distance);
    if (unit) *unit = ok ? 128 : 0;
    if (n_padded) *n_padded = E->np;
    if (k_padded) *k_padded = E->kp;
    return NMFX_OK;
}
int nmfx_mur_phase_a_head(nmfx_handle_t E, int distance, double lambda_w, int64_t j) {
    NMFX_MUR_PHASE_ENTRY(E, distance);
    int rc = mur_phase_enter(E, j, mur_keep(NMFX_EU)); if (rc) return rc;
    if (!mur_chunkable(E, distance)) { E->err = "phase_a_head: Euclidean loss on the split-bf16 path only (nmfx_mur_chunk_info)"; return NMFX_E_ARG; }
    return nmfx_mur_eu_phase_a_head_bf16(E, lambda_w, j);
}
int nmfx_mur_phase_a_cols(nmfx_handle_t E, int distance, int64_t c0, int64_t c1) {      // (a continuation of phase_a_head: no guard of its own)
    NMFX_MUR_PHASE_ENTRY(E, distance);
    if (!mur_chunkable(E, distance)) { E->err = "phase_a_cols: Euclidean loss on the split-bf16 path only (nmfx_mur_chunk_info)"; return NMFX_E_ARG; }
    NMFX_HIP(hipSetDevice(E->device));
    return nmfx_mur_eu_phase_a_cols_bf16(E, c0, c1);
}

int nmfx_mur_phase_b(nmfx_handle_t E, int distance, double lambda_h, int64_t min_iter, double tol1,
                     double tol2, int64_t j) {
    NMFX_MUR_PHASE_ENTRY(E, distance);
    int rc = mur_phase_enter(E, j, mur_keep(distance)); if (rc) return rc;
    E->run.ping_pong(j);
    if (E->kp > 128 && (distance == NMFX_EU || distance == NMFX_KL)) return nmfx_generic_mur_phase_b(E, distance, lambda_h, min_iter, tol1, tol2, j);
    if (distance == NMFX_EU)
        return mur_bf16(E) ? nmfx_mur_eu_phase_b_bf16(E, lambda_h, min_iter, tol1, tol2, j) : nmfx_mur_eu_phase_b(E, lambda_h, min_iter, tol1, tol2, j);
    if (distance == NMFX_KL)
        return mur_bf16(E) ? nmfx_mur_kl_phase_b_bf16(E, lambda_h, min_iter, tol1, tol2, j) : nmfx_mur_kl_phase_b(E, lambda_h, min_iter, tol1, tol2, j);
    E->err = "Unknown distance type."; return NMFX_E_ARG;
}

// Phase B by column slices (reduce-scatter / all-gather exchange, include/nmfx.h)
int nmfx_mur_slice_info(nmfx_handle_t E, int distance, int world, int64_t* cols, int64_t* elems) {
    NMFX_DENSE_ONLY(E);
    NMFX_EU_KL_ONLY(E, distance);
    if (!E || world < 1) return NMFX_E_ARG;
    const bool ok = mur_chunkable(E, distance) && E->xworld == world && (E->np / 64) % world == 0;
    const int64_t c = ok ? E->np / world : 0;
    if (cols) *cols = c;
    if (elems) *elems = c * E->kp;
    return NMFX_OK;
}
static int slice_args(nmfx_engine* E, int distance, int64_t c0, int64_t c1, const char* who) {
    if (!mur_chunkable(E, distance) || E->xworld <= 0) { E->err = std::string(who) + ": Euclidean loss on the split-bf16 path with nmfx_set_exchange_rank in force only (nmfx_mur_slice_info)"; return NMFX_E_ARG; }
    if (c0 < 0 || c1 < c0 || c1 > E->np || c0 % 64 || c1 % 64) { E->err = std::string(who) + ": column range must be whole 64-column blocks inside the padded n"; return NMFX_E_ARG; }
    return NMFX_OK;
}
int nmfx_mur_phase_b_slice(nmfx_handle_t E, int distance, double lambda_h, int64_t min_iter, double tol1, double tol2, int64_t j,
                           int64_t c0, int64_t c1) {
    NMFX_MUR_PHASE_ENTRY(E, distance);
    int rc = mur_phase_enter(E, j, mur_keep(NMFX_EU)); if (rc) return rc;
    if ((rc = slice_args(E, distance, c0, c1, "phase_b_slice"))) return rc;
    E->run.ping_pong(j);
    return nmfx_mur_eu_phase_b_slice_bf16(E, lambda_h, min_iter, tol1, tol2, j, (int)(c0 / 64), (int)((c1 - c0) / 64));
}
int nmfx_mur_phase_b_rest(nmfx_handle_t E, int distance, int64_t c0, int64_t c1) {      // (a continuation of phase_b_slice: no guard of its own)
    NMFX_MUR_PHASE_ENTRY(E, distance);
    int rc = slice_args(E, distance, c0, c1, "phase_b_rest"); if (rc) return rc;
    NMFX_HIP(hipSetDevice(E->device));
    return nmfx_mur_eu_phase_b_rest_bf16(E, (int)(c0 / 64), (int)((c1 - c0) / 64));
}

int nmfx_mur_finish_a(nmfx_handle_t E, int distance, int64_t j) {
    NMFX_MUR_PHASE_ENTRY(E, distance);
    int rc = mur_enter(E, j, 1, MUR_KEEP_CLOSING); if (rc) return rc;
    if (E->kp > 128 && (distance == NMFX_EU || distance == NMFX_KL)) return nmfx_generic_mur_finish_a(E, distance, j);
    if (distance == NMFX_EU) return nmfx_mur_eu_finish_a(E, j);
    if (distance == NMFX_KL) return nmfx_mur_kl_finish_a(E, j);
    E->err = "Unknown distance type."; return NMFX_E_ARG;
}

int nmfx_mur_finish_b(nmfx_handle_t E, int64_t min_iter, double tol1, double tol2, int64_t j) {
    NMFX_DENSE_ONLY(E);
    if (!E) return NMFX_E_ARG;
    int rc = mur_enter(E, j, 1, KEEP_FINISH_B, NMFX_FAM_NONE); if (rc) return rc;       // (the closing step of EVERY row-sharded solver, not only MUR's)
    return nmfx_finish_b(E, min_iter, tol1, tol2, j);
}

// IS on a dense handle: the tuned exact-f32 kernels of kernels_phase.hip, k <= 128, whatever the precision mode says
static int is_dense_ok(nmfx_engine* E, const char* who) {
    if (E->kp > 128) { E->err = std::string(who) + ": the Itakura-Saito divergence (IS) needs k <= 128 on a dense handle"; return NMFX_E_ARG; }
    if (mur_bf16(E) && E->note.find("Itakura-Saito") == std::string::npos)
        E->note += (E->note.empty() ? "" : "; ") + std::string("the Itakura-Saito divergence (IS) runs the exact-f32 kernels; the split-bf16 mode does not apply to it");
    return NMFX_OK;
}

// With per-entry weights (nmfx_upload_weights; dense, k <= 128 by construction) every loss runs kernels_phase.hip
static int weights_ok(nmfx_engine* E, int distance, const char* who) {
    if (distance != NMFX_EU && distance != NMFX_KL && distance != NMFX_IS) { E->err = "Unknown distance type."; return NMFX_E_ARG; }
    if (E->kp > 128) { E->err = std::string(who) + ": per-entry weights need k <= 128"; return NMFX_E_ARG; }
    return NMFX_OK;
}

// NMFX_BETA: kernels_phase.hip on a dense handle with k <= 128 (what nmfx_set_beta accepted), with or without weights
static int beta_ok(nmfx_engine* E, const char* who) {
    if (E->sp) { E->err = std::string(who) + ": the beta-divergence (NMFX_BETA) is not available on a sparse handle"; return NMFX_E_ARG; }
    if (E->kp > 128) { E->err = std::string(who) + ": the beta-divergence (NMFX_BETA) needs k <= 128"; return NMFX_E_ARG; }
    if (!E->beta_set) { E->err = std::string(who) + ": NMFX_BETA without a beta (nmfx_set_beta)"; return NMFX_E_STATE; }
    return NMFX_OK;
}

// The dense exact-f32 phase path (kernels_phase.hip) takes a call with NMFX_BETA, a dense handle with weights whatever the
// loss, and NMFX_IS on a dense handle -- asked in that order, each with its own guard.  *takes says whether it does.
static int dense_phase_path(nmfx_engine* E, int distance, const char* who, bool* takes) {
    *takes = true;
    if (distance == NMFX_BETA) return beta_ok(E, who);
    if (!E->sp && E->Om) return weights_ok(E, distance, who);
    if (!E->sp && distance == NMFX_IS) return is_dense_ok(E, who);
    *takes = false;
    return NMFX_OK;
}

// With nmfx_set_ard in force the penalty is the ARD one: NMFX_BETA alone, no lambda
static int ard_request_ok(nmfx_engine* E, int distance, double lambda_w, double lambda_h, const char* who) {
    if (!E->ard) return NMFX_OK;
    if (distance != NMFX_BETA) { E->err = std::string(who) + ": automatic relevance determination is set (nmfx_set_ard): only NMFX_BETA runs with it"; return NMFX_E_ARG; }
    if (lambda_w != 0.0 || lambda_h != 0.0) { E->err = std::string(who) + ": automatic relevance determination is set (nmfx_set_ard): lambda_w and lambda_h must be 0 (the penalty is the ARD one)"; return NMFX_E_ARG; }
    return NMFX_OK;
}

int nmfx_mur_run(nmfx_handle_t E, int distance, double lambda_w, double lambda_h, int64_t min_iter,
                 double tol1, double tol2, int64_t first, int64_t count) {
    if (!E) return NMFX_E_ARG;
    bool dense_phase;
    { int rc_a = ard_request_ok(E, distance, lambda_w, lambda_h, "mur_run"); if (rc_a) return rc_a; }
    { int rc_p = dense_phase_path(E, distance, "mur_run", &dense_phase); if (rc_p) return rc_p; }
    if (dense_phase) {
        int rc = mur_enter(E, first, count, NMFX_D_ard_valid); if (rc) return rc;
        E->run.mur_loss(distance);
        if ((rc = ard_ensure(E, E->W[first & 1]))) return rc;             // lambda_0, or the relevances a new beta voided
        for (int64_t j = first; j < first + count && !rc; ++j) {
            if ((rc = nmfx_mur_dense_phase_a(E, distance, lambda_w, j))) break;
            E->run.ping_pong(j);
            rc = nmfx_mur_dense_phase_b(E, distance, lambda_h, min_iter, tol1, tol2, j);
        }
        return rc;
    }
    if (E->sp) return nmfx_sparse_mur_run(E, distance, lambda_w, lambda_h, min_iter, tol1, tol2, first, count);
    // (the guard of the run as a whole keeps what a closing step keeps: what the loss voids is up to the phases it goes through)
    int rc = mur_enter(E, first, count, MUR_KEEP_CLOSING); if (rc) return rc;
    E->run.mur_loss(NMFX_EU);
    E->run.fused_pack = true;        // nothing is exchanged between the phases here
    for (int64_t j = first; j < first + count && !rc; ++j) {
        if ((rc = nmfx_mur_phase_a(E, distance, lambda_w, j))) break;
        rc = nmfx_mur_phase_b(E, distance, lambda_h, min_iter, tol1, tol2, j);
    }
    E->run.fused_pack = false;
    return rc;
}

int nmfx_mur_finish(nmfx_handle_t E, int distance, int64_t min_iter, double tol1, double tol2,
                    int64_t iters_done) {
    int rc;
    bool dense_phase = false;
    if (E && (rc = ard_request_ok(E, distance, 0.0, 0.0, "mur_finish"))) return rc;
    if (E && (rc = dense_phase_path(E, distance, "mur_finish", &dense_phase))) return rc;
    if (dense_phase) {
        if ((rc = mur_enter(E, iters_done, 1, MUR_KEEP_CLOSING | NMFX_D_ard_valid))) return rc;
        E->run.mur_loss(distance);
        if ((rc = ard_ensure(E, E->W[iters_done & 1]))) return rc;
        if ((rc = nmfx_mur_dense_finish_a(E, distance, iters_done))) return rc;
        return E->ard ? nmfx_ard_finish_b(E, min_iter, tol1, tol2, iters_done) : nmfx_finish_b(E, min_iter, tol1, tol2, iters_done);
    }
    if (E && E->sp) return nmfx_sparse_mur_finish(E, distance, min_iter, tol1, tol2, iters_done);
    if ((rc = nmfx_mur_finish_a(E, distance, iters_done))) return rc;
    return nmfx_mur_finish_b(E, min_iter, tol1, tol2, iters_done);
}

// ---- fold-in (version 370; kernels_phase.hip) ----------------
// What both entry points refuse, nothing launched
static const char* const FOLDIN_NOTE = "fold-in (nmfx_foldin_run) runs the exact-f32 kernels whatever the precision mode";
static int foldin_ok(nmfx_engine* E, int distance, const char* who) {
    if (E->sp) { E->err = std::string(who) + ": fold-in is not available on a sparse handle (dense V, k <= 128)"; return NMFX_E_ARG; }
    if (E->kp > 128) { E->err = std::string(who) + ": fold-in needs k <= 128"; return NMFX_E_ARG; }
    if (distance != NMFX_EU && distance != NMFX_KL && distance != NMFX_IS && distance != NMFX_BETA) { E->err = "Unknown distance type."; return NMFX_E_ARG; }
    if (distance == NMFX_BETA && !E->beta_set) { E->err = std::string(who) + ": NMFX_BETA without a beta (nmfx_set_beta)"; return NMFX_E_STATE; }
    if (E->ard) { E->err = std::string(who) + ": automatic relevance determination is set (nmfx_set_ard): fold-in does not use the relevances, nmfx_clear_ard first"; return NMFX_E_STATE; }
    if (!E->have_v || !E->have_f) { E->err = std::string(who) + ": upload V and set factors first"; return NMFX_E_STATE; }
    return NMFX_OK;
}

// Both entry points: the refusals, the guard (H moves, nothing derived from it is kept), then W stays in the buffer that holds
// it (after nmfx_set_factors: W[0]) -- *W
static int foldin_enter(nmfx_engine* E, int distance, const char* who, int64_t first, int64_t count, const float** W) {
    int rc;
    if ((rc = foldin_ok(E, distance, who))) return rc;
    if ((rc = mur_enter(E, first, count, NMFX_D_NONE))) return rc;
    E->run.mur_loss(distance);
    E->run.w_in_place = true;
    if (E->note.find(FOLDIN_NOTE) == std::string::npos) E->note += (E->note.empty() ? "" : "; ") + std::string(FOLDIN_NOTE);
    *W = E->W[E->run.wsel];
    return NMFX_OK;
}

int nmfx_foldin_run(nmfx_handle_t E, int distance, double lambda_h, int64_t min_iter, double tol1, double tol2, int64_t first, int64_t count) {
    if (!E) return NMFX_E_ARG;
    const float* W;
    int rc = foldin_enter(E, distance, "foldin_run", first, count, &W);
    for (int64_t j = first; j < first + count && !rc; ++j) rc = nmfx_foldin_step(E, distance, lambda_h, min_iter, tol1, tol2, j, W);
    return rc;
}

int nmfx_foldin_finish(nmfx_handle_t E, int distance, int64_t min_iter, double tol1, double tol2, int64_t iters_done) {
    if (!E) return NMFX_E_ARG;
    const float* W;
    int rc = foldin_enter(E, distance, "foldin_finish", iters_done, 1, &W); if (rc) return rc;
    if ((rc = nmfx_foldin_finish_a(E, distance, W))) return rc;
    return nmfx_finish_b(E, min_iter, tol1, tol2, iters_done);
}

// ---- profiling (scopes and counts on dense and sparse handles alike; nmfx_profile_repeat is dense-only) -----
static void drain_profile(nmfx_engine* E) {
    if (E->prof_pending.empty()) return;
    hipStreamSynchronize(E->stream);
    for (auto& t : E->prof_pending) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, std::get<1>(t), std::get<2>(t)) == hipSuccess) {
            ProfSlot& s = E->prof_slots[std::get<0>(t)];
            s.ms += ms; s.n += 1;
        }
        hipEventDestroy(std::get<1>(t)); hipEventDestroy(std::get<2>(t));
    }
    E->prof_pending.clear();
}

int nmfx_profile_enable(nmfx_handle_t E, int on) {
    if (!E) return NMFX_E_ARG;
    drain_profile(E);
    E->prof = on != 0;
    return NMFX_OK;
}

int nmfx_profile_get(nmfx_handle_t E, const char* name, double* total_ms, int64_t* launches) {
    if (!E || !name) return NMFX_E_ARG;
    drain_profile(E);
    auto it = E->prof_slots.find(name);
    if (total_ms) *total_ms = it == E->prof_slots.end() ? 0.0 : it->second.ms;
    if (launches) *launches = it == E->prof_slots.end() ? 0 : it->second.n;
    return NMFX_OK;
}

// `reps` back-to-back launches of ONE product kernel of the current state between a single pair of HIP events:
// the per-launch time of the dominant kernel without an event (= a command-processor barrier) in front of
// every launch, which costs the W phase ~10 us that no real iteration pays.
int nmfx_profile_repeat(nmfx_handle_t E, const char* which, int distance, int reps, double* ms_per_launch) {
    NMFX_DENSE_ONLY(E);
    NMFX_EU_KL_ONLY(E, distance);
    if (!E || !which || reps <= 0 || !ms_per_launch) return NMFX_E_ARG;
    const std::string w(which);
    int rc = mur_enter(E, 0, 0, KEEP_FINISH_B, w.rfind("ao_", 0) == 0 || w.rfind("sk_", 0) == 0 ? NMFX_FAM_NONE : NMFX_FAM_MUR); if (rc) return rc;
    const bool wph = w == "wphase";
    // r4, the two V-sized products of AO-ADMM at k padded to 128 (after at least one nmfx_aoadmm_run on the handle, so that the images
    // and Gram slabs exist): "ao_hphase" / "ao_wphase" = the (row block) x (split) launches, "sk_hphase" / "sk_wphase" = the stream-K
    // form without a side job, "..._side" = with the inversion of the Gram slabs beside it
    const bool ao = w.rfind("ao_", 0) == 0 || w.rfind("sk_", 0) == 0;
    if (ao && !(E->precision == 1 && E->kp == 128 && E->bf_ready && E->HThi)) { E->err = "profile_repeat: AO-ADMM products need a split-bf16 k = 128 run first"; return NMFX_E_STATE; }
    if (!ao && !wph && w != "hphase") { E->err = "profile_repeat: which must be wphase or hphase"; return NMFX_E_ARG; }
    if (distance != NMFX_EU && distance != NMFX_KL) { E->err = "Unknown distance type."; return NMFX_E_ARG; }
    const bool bf = mur_bf16(E);
    const bool kl = distance == NMFX_KL;
    if (bf) {
        if (!E->bf_ready) E->run.wsel = 0;
        if ((rc = nmfx_bf16_prepare(E))) return rc;
        if (kl && (rc = nmfx_bf16_images_h(E, true))) return rc;          // H^T images: the Z operand of the KL H phase
    }
    const bool was = E->prof;
    E->prof = false;
    hipEvent_t a, b;
    NMFX_HIP(hipEventCreate(&a)); NMFX_HIP(hipEventCreate(&b));
    for (int i = -2; i < reps && !rc; ++i) {                               // two untimed launches first
        if (i == 0) NMFX_HIP(hipEventRecord(a, E->stream));
        if (ao) {
            const bool side = w.find("_side") != std::string::npos, hside = w.find("hphase") != std::string::npos;
            if (w.rfind("ao_", 0) == 0) rc = hside ? nmfx_bf16_vtw(E, true, "hphase", false, 3) : nmfx_bf16_vht(E, false, 0, "wphase_noobj", false, 3);
            else rc = nmfx_bf16_sk_product(E, hside ? 0 : 1, hside, side ? (hside ? E->G_part : E->HHt_part) : nullptr, hside ? 64 : 32, -1.0,
                                           hside ? "hphase" : "wphase_noobj");
        }
        else if (bf) rc = wph ? nmfx_bf16_vht(E, true, E->run.wsel, "wphase", kl, 3) : nmfx_bf16_vtw(E, false, "hphase", kl, 3);
        else if (kl) { E->err = "profile_repeat: KL only in the split-bf16 mode"; rc = NMFX_E_ARG; }
        else rc = wph ? nmfx_launch_wphase(E, E->W[E->run.wsel], true, true) : nmfx_launch_hphase(E, E->W[E->run.wsel], nmfx_hphase_can_fuse_gram(E));
    }
    E->prof = was;
    if (rc) { hipEventDestroy(a); hipEventDestroy(b); return rc; }
    NMFX_HIP(hipEventRecord(b, E->stream));
    NMFX_HIP(hipEventSynchronize(b));
    float ms = 0.f;
    NMFX_HIP(hipEventElapsedTime(&ms, a, b));
    hipEventDestroy(a); hipEventDestroy(b);
    *ms_per_launch = (double)ms / reps;
    return NMFX_OK;
}

int nmfx_profile_reset(nmfx_handle_t E) {
    if (!E) return NMFX_E_ARG;
    drain_profile(E);
    E->prof_slots.clear();
    return NMFX_OK;
}

}  // extern "C"
