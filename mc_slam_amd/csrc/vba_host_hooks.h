// vba_host_hooks.h -- host side of the library, part 6: the vba_debug_* hooks of the hooks flavour.
#pragma once

// ---- test / diagnostic hooks: NOT part of include/vislam_ba.h and not in the shipped library.  `make` builds a second flavour,
// libvislam_ba_hooks.so (-DVBA_TEST_HOOKS), that the tests load when they need to look inside (tests/test_abi_exports.py checks
// that libvislam_ba.so exports exactly the header).
#ifdef VBA_TEST_HOOKS
namespace {
// a path override of the handle, pushed to the lanes vba_batch_solve has created already (new lanes and arenas copy the parent's)
using vba_host::PathOverrides;
int set_path_opt(void* handle, int PathOverrides::*f, int value) {
    Handle* h = reinterpret_cast<Handle*>(handle);
    if (!h) return -1;
    h->ov.path.*f = value;
    for (Handle* l : h->lanes) l->ov.path = h->ov.path;
    return 0;
}
}  // namespace
extern "C" {
// test/debug hook (not part of include/vislam_ba.h): raw copy out of one device buffer of the last batch
int vba_debug_copy(void* handle, int32_t buf_id, uint64_t offset_bytes, void* dst, uint64_t nbytes) {
    Handle* h = reinterpret_cast<Handle*>(handle);
    if (!h || buf_id < 0 || buf_id >= BUF_N) return -1;
    const DevBuf& b = h->buf[buf_id];
    if (offset_bytes + nbytes > (b.view ? b.view_bytes : b.cap)) return -1;
    (void)hipSetDevice(h->device);
    return hipMemcpy(dst, reinterpret_cast<char*>(b.ptr()) + offset_bytes, nbytes, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -1;
}
// diagnostic (bench.py --workload c3s): tile products of window w's symbolic factorisation under both elimination orders and the
// order chosen: out[5] = {V/Bias-first, keyframe by keyframe, chosen order, products of the chosen lists, two-sided V/Bias-first}
int vba_debug_tile_products(void* handle, int32_t w, int64_t* out) {
    Handle* h = reinterpret_cast<Handle*>(handle);
    if (!h || !out || w < 0 || w >= h->n_win || (size_t)w >= h->win_tiles.size()) return -1;
    out[0] = h->win_prod_order[3 * (size_t)w]; out[1] = h->win_prod_order[3 * (size_t)w + 1];
    out[2] = h->desc[w].order; out[3] = h->win_tiles[w]; out[4] = h->win_prod_order[3 * (size_t)w + 2];
    return 0;
}
int vba_debug_set_streams(void* handle, int32_t n) {
    Handle* h = reinterpret_cast<Handle*>(handle);
    if (!h) return -1;
    h->ov.streams = n;
    return 0;
}
// every window reads the stop flag as 1 from its n-th terminate() poll on (n < 0: off); the oracle's vba_oracle_solve_ex counts alike
int vba_debug_set_stop_after(void* handle, int32_t n) { return set_path_opt(handle, &PathOverrides::stop_after, n); }
// 1: the first form of the fused factorisation step (v_readlane broadcasts, panel solves after the diagonal tile); anything else: k_chol_step4
int vba_debug_set_chol_step(void* handle, int32_t form) { return set_path_opt(handle, &PathOverrides::chol_step, form); }
int vba_debug_set_lin_fallback(void* handle, int32_t on) { return set_path_opt(handle, &PathOverrides::lin_fallback, on); }
int vba_debug_set_ll_min(void* handle, int32_t n) { return set_path_opt(handle, &PathOverrides::ll_min, n); }
int vba_debug_set_chunking(void* handle, int32_t chunk, int32_t lanes) {
    Handle* h = reinterpret_cast<Handle*>(handle);
    if (!h) return -1;
    h->ov.chunk = chunk;
    h->ov.lanes = lanes;
    return 0;
}
// test hook: while on, the workers of vba_batch_submit start no upload (submitted tickets stay pending: observable without timing)
int vba_debug_async_hold(void* handle, int32_t on) {
    Handle* h = reinterpret_cast<Handle*>(handle);
    if (!h) return -1;
    AsyncState& A = async_state(h);
    {
        std::lock_guard<std::mutex> lk(A.mu);
        A.hold = on != 0;
    }
    A.cv.notify_all();
    return 0;
}
int vba_debug_buf_id(const char* name) {
#define VBA_BUF_NAME(id) #id,
    static const char* names[BUF_N] = {VBA_BUFFERS(VBA_BUF_NAME)};
#undef VBA_BUF_NAME
    for (int i = 0; i < BUF_N; i++)
        if (!strcmp(names[i], name)) return i;
    return -1;
}

// chain columns of the factorisation (vba_chain.h): 0 = one launch per block column everywhere, 1 = the default policy
int vba_debug_set_chain(void* handle, int32_t on) { return set_path_opt(handle, &PathOverrides::no_chain, on ? 0 : 1); }

// the A/B paths read from the environment, per handle: "schur_split", "trsv_old", "pcg_jacobi" (value 0 / 1); and "lin_probe", which
// no variable sets: 0 off, 1 on at any batch size, 2 a chi2-only probe wherever one may run, -1 back to the default (plan_lin_probe).
// A window's counters are the last two ints of its WinCtrl (vba_debug_copy of buffer "CTRL"; size: vba_debug_window_layout [13]):
// n_probe at sizeof(WinCtrl) - 8, n_redo at - 4
int vba_debug_set_path(void* handle, const char* name, int32_t value) {
    if (!name) return -1;
    if (!strcmp(name, "lin_probe")) return (value < -1 || value > 2) ? -1 : set_path_opt(handle, &PathOverrides::lin_probe, value);
    int PathOverrides::*f = !strcmp(name, "schur_split") ? &PathOverrides::schur_split : !strcmp(name, "trsv_old") ? &PathOverrides::trsv_old
                          : !strcmp(name, "pcg_jacobi") ? &PathOverrides::pcg_jacobi : nullptr;
    return f ? set_path_opt(handle, f, value ? 1 : 0) : -1;
}

// During the next vba_batch_run: at its call-th enqueue_solve_iteration (0-based, both stages), copy (a) the state and the control
// blocks before the Schur launches, (b) S and the reduced rhs after them, (c) the factor, y and x_c after the triangular solves,
// (d) the state after the update.  Refused (at the run) when the batch runs as more than one window group.
int vba_debug_capture(void* handle, int32_t call) {
    Handle* h = reinterpret_cast<Handle*>(handle);
    if (!h || call < 0) return -1;
    if (!h->uploaded || h->desc.empty()) return fail(h, "vba_debug_capture before vba_batch_upload");
    h->cap_call = call;
    h->cap_done = 0;
    return 0;
}
// window w's slice of captured item `what` (CAP_*), nbytes exactly its size
int vba_debug_capture_get(void* handle, int32_t what, int32_t w, void* dst, uint64_t nbytes) {
    Handle* h = reinterpret_cast<Handle*>(handle);
    if (!h || !dst || what < 0 || what >= CAP_N || w < 0 || w >= (int)h->desc.size() || !h->cap_done) return -1;
    if (h->solver == VBA_SOLVER_PCG && (what == CAP_LF_C || what == CAP_YV_C)) return fail(h, "vba_debug_capture_get: PCG has no factor");
    const WinDesc& d = h->desc[w];
    size_t off = 0, len = 0;
    switch (what) {
        case CAP_POSE_A: case CAP_POSE_D: off = 56 * (size_t)d.kf0; len = 56 * (size_t)d.n_kf; break;
        case CAP_VEL_A: case CAP_VEL_D: off = 24 * (size_t)d.kf0; len = 24 * (size_t)d.n_kf; break;
        case CAP_BIAS_A: case CAP_BIAS_D: off = 96 * (size_t)d.kf0; len = 96 * (size_t)d.n_kf; break;
        case CAP_PT_A: case CAP_PT_D: off = 24 * (size_t)d.pt0; len = 24 * (size_t)d.n_pt; break;
        case CAP_CTRL_A: off = sizeof(WinCtrl) * (size_t)w; len = sizeof(WinCtrl); break;
        case CAP_LVL_A: off = (size_t)d.obs0; len = (size_t)d.n_obs; break;
        case CAP_VARACT_A: off = 4 * (size_t)d.vec0; len = 4 * (size_t)d.nS; break;
        case CAP_S_B: case CAP_LF_C: off = 8 * (size_t)d.S0; len = 8 * (size_t)d.nS * d.nS; break;
        default: off = 8 * (size_t)d.vec0; len = 8 * (size_t)d.nS; break;   // VEC_B, YV_C, VEC_C
    }
    if (nbytes != len || off + len > h->cap_bytes[what] || off + len > h->cap[what].cap) return -1;
    (void)hipSetDevice(h->device);
    return hipMemcpy(dst, reinterpret_cast<char*>(h->cap[what].p) + off, len, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -1;
}
// Window w's layout of the reduced system, n_out int64 entries:
//   [0] nS [1] nb [2] pdim [3] n_free [4] order [5] nc [6] nc_split [7] l_packed [8] regime_n [9] n_win
//   [10..12] kernel paths of the captured iteration (Schur, factor, triangular solve: CAP_SCHUR_*, CAP_FACTOR_*, CAP_TRSV*)
//   [13] sizeof(WinCtrl) [14] solver is PCG [15] pcg_tri
//   [16..19] byte offsets in WinCtrl of stage, active, robust_vis (int) and lambda (double)
//   [20, 20 + pdim n_free) row of S of dof r of free keyframe a at 20 + pdim a + r (vpos), then pad0[3], padn[3]
int vba_debug_window_layout(void* handle, int32_t w, int64_t* out, int64_t n_out) {
    Handle* h = reinterpret_cast<Handle*>(handle);
    if (!h || !out || w < 0 || w >= (int)h->desc.size()) return -1;
    const WinDesc& d = h->desc[w];
    if (n_out < 20 + (int64_t)d.pdim * d.n_free + 6) return -1;
    out[0] = d.nS; out[1] = d.nb; out[2] = d.pdim; out[3] = d.n_free; out[4] = d.order; out[5] = d.nc; out[6] = d.nc_split;
    out[7] = h->B.l_packed; out[8] = h->up.n_win; out[9] = h->n_win;
    for (int i = 0; i < 3; i++) out[10 + i] = h->cap_path[i];
    out[13] = sizeof(WinCtrl);
    out[14] = h->solver == VBA_SOLVER_PCG; out[15] = h->rp.pcg_tri;
    out[16] = offsetof(WinCtrl, stage); out[17] = offsetof(WinCtrl, active); out[18] = offsetof(WinCtrl, robust_vis);
    out[19] = offsetof(WinCtrl, lambda);
    int64_t* vp = out + 20;
    for (int a = 0; a < d.n_free; a++)
        for (int r = 0; r < d.pdim; r++) vp[d.pdim * a + r] = vba_host::vpos(d, a, r);
    for (int q = 0; q < 3; q++) { vp[d.pdim * d.n_free + q] = d.pad0[q]; vp[d.pdim * d.n_free + 3 + q] = d.padn[q]; }
    return 0;
}
// The plan of the uploaded batch and of its last run (vba_host_plan.h: UploadPlan, RunPlan) as PLAN_INTS integers, in the order
// documented at vba_host::plan_ints; before the first run of an upload the RunPlan entries are -1
int vba_debug_plan(void* handle, int64_t* out, int64_t n_out) {
    Handle* h = reinterpret_cast<Handle*>(handle);
    if (!h || !out || n_out < vba_host::PLAN_INTS || !h->uploaded) return -1;
    long long v[vba_host::PLAN_INTS];
    vba_host::plan_ints(h->up, h->rp, v);
    for (int i = 0; i < vba_host::PLAN_INTS; i++) out[i] = (i < vba_host::PLAN_UPLOAD_INTS || h->ran) ? v[i] : -1;
    return 0;
}
// From the captured factor of window w: L (unit lower) with D on its diagonal, dense nS x nS row-major, exactly the tiles the
// triangular solves read (the diagonal tiles and the panel tiles of every block column); zeros elsewhere and above the diagonal
int vba_debug_factor_dense(void* handle, int32_t w, double* out, int64_t n_out) {
    Handle* h = reinterpret_cast<Handle*>(handle);
    if (!h || !out || w < 0 || w >= (int)h->desc.size() || !h->cap_done || h->solver == VBA_SOLVER_PCG) return -1;
    const WinDesc& d = h->desc[w];
    const size_t n = d.nS;
    if (n_out != (int64_t)(n * n) || d.nb * VBA_NB != d.nS) return -1;
    std::vector<double> lf(n * n);
    std::vector<int> pb(d.nb + 1);
    if (vba_debug_capture_get(handle, CAP_LF_C, w, lf.data(), n * n * 8)) return -1;
    (void)hipSetDevice(h->device);
    auto avail = [&](int id) { const DevBuf& b = h->buf[id]; return b.view ? b.view_bytes : b.cap; };
    if (((size_t)d.tl_step0 + d.nb + 1) * 4 > avail(BUF_TLPANB)) return -1;
    if (hipMemcpy(pb.data(), dp<int>(h, BUF_TLPANB) + d.tl_step0, (d.nb + 1) * 4, hipMemcpyDeviceToHost) != hipSuccess) return -1;
    for (int k = 0; k < d.nb; k++)
        if (pb[k] < 0 || pb[k + 1] < pb[k]) return -1;
    std::vector<int> pan(std::max(1, pb[d.nb]));
    if (((size_t)d.tl_pan0 + pb[d.nb]) * 4 > avail(BUF_TLPAN)) return -1;
    if (pb[d.nb] > 0 && hipMemcpy(pan.data(), dp<int>(h, BUF_TLPAN) + d.tl_pan0, (size_t)pb[d.nb] * 4, hipMemcpyDeviceToHost) != hipSuccess) return -1;
    std::fill(out, out + n * n, 0.0);
    const bool pk = h->B.l_packed;
    auto tile = [&](int I, int J) {
        for (int r = 0; r < VBA_NB; r++)
            for (int c = 0; c < VBA_NB; c++) {
                const size_t gr = (size_t)I * VBA_NB + r, gc = (size_t)J * VBA_NB + c;
                if (gc > gr) continue;
                const int pr = (((((r >> 4) * 4 + (c >> 3)) * 64) + ((c & 3) * 16 + (r & 15))) * 2) + ((c >> 2) & 1);   // ll_pk
                out[gr * n + gc] = pk ? lf[1024 * ((size_t)I * d.nb + J) + pr] : lf[gr * n + gc];
            }
    };
    for (int k = 0; k < d.nb; k++) {
        tile(k, k);
        for (int i = pb[k]; i < pb[k + 1]; i++) {
            const int I = pan[i];
            if (I <= k || I >= d.nb) return -1;
            tile(I, k);
        }
    }
    return 0;
}
}  // extern "C"
#endif  // VBA_TEST_HOOKS
