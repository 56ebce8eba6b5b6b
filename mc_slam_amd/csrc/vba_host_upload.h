// vba_host_upload.h -- host side of the library, part 2: vba_batch_upload.  do_upload drives named stages: check and size, per chunk
// of windows {structure pool, describe, grow staging, pack pool, incremental copy}, allocate and copy, the results block of a few
// windows, zero and pad, bind_batch, enqueue_structure_build.  The description of a window is plain C++ (vba_host_layout.h).
#pragma once

namespace {

// an array whose freshly packed tail is copied after every packing pass (upload_inc_push)
struct IncCopy { int id; const char* base; size_t esz, total, done; };

// what the stages of one upload share
struct Upload {
    int n = 0;
    vba_problem* const* probs = nullptr;
    vba_host::DescribeOpts opts;
    int n_threads = 1;
    vba_host::BatchCursor cur;
    vba_host::BatchTables tab;
    std::vector<Structure> sts;   // the structures of the chunk being worked on
    std::vector<IncCopy> inc;
    size_t tot_kf = 0, tot_pt = 0, tot_obs = 0, tot_mask = 0;
    double t_struct = 0;
};

// the stop word the windows of a batch (or of one of its window groups) poll
int* stop_word_of(Handle* h, const Batch& B) { return h->up.dev_stop ? B.alive_dev + 1023 : h->stop_dev; }

// check and size: the handle's per-batch state, the options of the batch, one allocation per concatenated array
int upload_begin(Handle* h, Upload& U) {
    const int n = U.n;
    vba_problem* const* probs = U.probs;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->up_stream));   // (an upload that failed half way may still have copies out of the staging in flight)
    h->uploaded = false;
    h->n_win = n;
    U.opts.pcg = probs[0] && probs[0]->solver == VBA_SOLVER_PCG;
    U.opts.pcg_rows = PCG_ROWS;
    h->up = vba_host::plan_upload(n, U.opts.pcg, h->ov, vba_host::current_knobs());
    U.opts.chain_on = h->up.chain_on;
    for (auto& b : h->buf) { b.view = nullptr; b.view_bytes = 0; }
    h->pending.clear();
    h->desc.assign(n, WinDesc());
    h->win_tiles.assign(n, 0);
    h->win_prod_order.assign(3 * (size_t)n, -1);
    h->geom = LaunchGeom();
    Staging& G = h->stg;
    G.each([](auto& v) { v.clear(); });
    static const int n_threads = host_threads();
    U.n_threads = n_threads;
    {   // one allocation per concatenated array instead of the doubling growth of std::vector
        size_t skf = 0, spt = 0, sobs = 0, simu = 0, spair = 0, smask = 0;
        for (int w = 0; w < n; w++) {
            const vba_problem* P = probs[w];
            if (!P || !vba_host::window_sizes_ok(P)) continue;   // (refused below)
            skf += P->n_kf; spt += P->n_pt; sobs += P->n_obs; simu += P->n_imu;
            spair += (size_t)P->n_kf_free * (P->n_kf_free + 1) / 2;
            smask += (size_t)P->n_pt * (size_t)((P->n_kf + 63) / 64);
        }
        U.tot_kf = skf; U.tot_pt = spt; U.tot_obs = sobs; U.tot_mask = smask;
        G.pose.reserve(7 * skf); G.vel.reserve(3 * skf); G.bias.reserve(12 * skf); G.kffix.reserve(skf);
        G.pt.reserve(3 * spt); G.ptref.reserve(spt); G.ptobs.reserve(spt + n); G.lmask.reserve(smask);
        G.obskf.reserve(sobs); G.uv.reserve(2 * sobs); G.ow.reserve(sobs);
        G.imui.reserve(simu); G.imuj.reserve(simu); G.meas.reserve(61 * simu); G.info.reserve(81 * simu);
        G.pair_a.reserve(spair); G.pair_b.reserve(spair); G.offpair.reserve(spair); G.pairmask.reserve(spair);
        G.pimu_begin.reserve(spair + n);
    }
    // The bulk of a window (observations, landmarks, masks: 1 MB of the 1.06 MB of a C3 window) crosses PCIe WHILE the host works on the
    // next windows: after every packing pass the freshly packed tail of these arrays is copied (their final sizes are known from
    // the pre-pass above, the pinned staging is never re-allocated under a copy).  Before: validate + symbolic (5.4 ms per 384
    // windows), pack (5.0), then ONE copy per array (7.5) one after the other -- the link idle for the first half, the host for the second.
    if (h->up.inc_copy) {
        auto reg = [&](int id, const void* base, size_t esz, size_t total) -> int {
            if (dalloc(h, id, total * esz)) return -1;
            U.inc.push_back({id, reinterpret_cast<const char*>(base), esz, total, 0});
            return 0;
        };
        if (reg(BUF_OBSUV, G.uv.data(), 16, U.tot_obs) || reg(BUF_OBSW, G.ow.data(), 8, U.tot_obs) || reg(BUF_OBSKF, G.obskf.data(), 4, U.tot_obs) ||
            reg(BUF_PT0, G.pt.data(), 24, U.tot_pt) || reg(BUF_PTREF, G.ptref.data(), 4, U.tot_pt) || reg(BUF_LMASK, G.lmask.data(), 8, U.tot_mask) ||
            reg(BUF_POSE0, G.pose.data(), 56, U.tot_kf) || reg(BUF_BIAS0, G.bias.data(), 96, U.tot_kf) || reg(BUF_VEL0, G.vel.data(), 24, U.tot_kf)) return -1;
    }
    return 0;
}

// (1) the per-window structure (item lists, IMU lists, symbolic tile factorisation: 0.7 ms for a C3 window) on a pool of host threads
int upload_structures(Handle* h, Upload& U, int chunk0, int cn) {
    for (int q = 0; q < cn; q++)
        if (!U.probs[chunk0 + q]) return fail(h, "null problem");
    U.sts.assign(cn, Structure());
    std::atomic<int> bad(0);
    const double ts0 = now_ms();
    host_parallel_for(h, cn, std::min(U.n_threads, cn), [&](int q) {
        const vba_problem* Q = U.probs[chunk0 + q];
        if (!vba_host::window_sizes_ok(Q)) return;  // reported by upload_describe
        if (build_structure(h, Q, U.sts[q], h->up.two_sided)) bad.store(1);
    });
    U.t_struct += now_ms() - ts0;
    if (bad.load()) return -1;
    if (chunk0 == 0) {   // tile lists: extrapolate from the first chunk
        size_t tp = 0;
        for (auto& x : U.sts) tp += x.tpairs.size() + x.klist.size();
        U.tab.tlpair.reserve((size_t)(1.1 * tp / cn * U.n) + 1024); U.tab.tlk.reserve((size_t)(1.1 * tp / cn * U.n) + 1024);
    }
    return 0;
}

// (2) refusals, descriptors and offsets in window order on this thread
int upload_describe(Handle* h, Upload& U, int chunk0, int cn) {
    for (int w = chunk0; w < chunk0 + cn; w++) {
        const Structure& st = U.sts[w - chunk0];
        const char* msg = vba_host::check_window(U.probs[w], U.probs[0]);
        if (!msg) msg = vba_host::describe_window(U.probs[w], st, U.opts, U.cur, h->geom, U.tab, h->desc[w]);
        if (msg) return fail(h, msg);
        h->win_tiles[w] = (int)st.tpairs.size();
        if (U.n == 1) h->one_sb = st.step_begin;
        for (int q = 0; q < 3; q++) h->win_prod_order[3 * (size_t)w + q] = st.prod_order[q];
    }
    return 0;
}

// (3) the concatenated arrays grown once, for the nw windows described so far
int upload_grow_staging(Handle* h, const Upload& U, int nw) {
    Staging& G = h->stg;
    const vba_host::BatchCursor& c = U.cur;
    G.pose.resize(7 * (size_t)c.kf0); G.vel.resize(3 * (size_t)c.kf0); G.bias.resize(12 * (size_t)c.kf0); G.kffix.resize(c.kf0);
    G.pt.resize(3 * (size_t)c.pt0); G.ptref.resize(c.pt0); G.lmask.resize((size_t)c.mask0); G.ptobs.resize((size_t)c.pt0 + nw);
    G.obskf.resize(c.obs0); G.uv.resize(2 * (size_t)c.obs0); G.ow.resize(c.obs0);
    G.imui.resize(c.imu0); G.imuj.resize(c.imu0); G.meas.resize(61 * (size_t)c.imu0); G.info.resize(81 * (size_t)c.imu0);
    G.pair_a.resize(c.pair0); G.pair_b.resize(c.pair0); G.offpair.resize(c.pair0); G.pairmask.resize(c.pair0);
    G.pimu_begin.resize((size_t)c.pair0 + nw);
    G.pimu.resize(2 * (size_t)c.pimu0);
    if (!G.ok()) return fail(h, "out of pinned host memory (upload staging)");
    return 0;
}

// (4) one window's arrays copied to its offsets (2.2 MB per C3 window)
void pack_window(Staging& G, const vba_problem* P, const WinDesc& d, Structure& st, bool pristine) {
    const int w = d.win;
    auto put = [](auto* dst, const auto* src, size_t cnt) { if (cnt) memcpy(dst, src, cnt * sizeof(*dst)); };
    put(G.pose.data() + 7 * (size_t)d.kf0, P->kf_pose, 7 * (size_t)d.n_kf);
    for (int k = 0; k < d.n_kf; k++) G.kffix[d.kf0 + k] = P->kf_fix ? (unsigned char)(P->kf_fix[k] & 7) : 0;
    if (P->kf_vel) put(G.vel.data() + 3 * (size_t)d.kf0, P->kf_vel, 3 * (size_t)d.n_kf);
    else std::fill_n(G.vel.data() + 3 * (size_t)d.kf0, 3 * (size_t)d.n_kf, 0.0);
    if (P->kf_bias) put(G.bias.data() + 12 * (size_t)d.kf0, P->kf_bias, 12 * (size_t)d.n_kf);
    else std::fill_n(G.bias.data() + 12 * (size_t)d.kf0, 12 * (size_t)d.n_kf, 0.0);
    put(G.pt.data() + 3 * (size_t)d.pt0, P->pt, 3 * (size_t)d.n_pt);
    if (P->pt_ref_kf) put(G.ptref.data() + d.pt0, P->pt_ref_kf, d.n_pt);
    else std::fill_n(G.ptref.data() + d.pt0, d.n_pt, 0);
    put(G.ptobs.data() + d.pt0 + w, P->pt_obs_begin, (size_t)d.n_pt + 1);
    put(G.obskf.data() + d.obs0, P->obs_kf, d.n_obs);
    put(G.lmask.data() + d.mask0, st.lmask.data(), st.lmask.size());
    put(G.uv.data() + 2 * (size_t)d.obs0, P->obs_uv, 2 * (size_t)d.n_obs);
    put(G.ow.data() + d.obs0, P->obs_w, d.n_obs);
    if (d.n_imu) {
        put(G.imui.data() + d.imu0, P->imu_kf_i, d.n_imu);
        put(G.imuj.data() + d.imu0, P->imu_kf_j, d.n_imu);
        put(G.meas.data() + 61 * (size_t)d.imu0, P->imu_meas, 61 * (size_t)d.n_imu);
        put(G.info.data() + 81 * (size_t)d.imu0, P->imu_info_prv, 81 * (size_t)d.n_imu);
    }
    put(G.pair_a.data() + d.pair0, st.pair_a.data(), d.n_pairs);
    put(G.pair_b.data() + d.pair0, st.pair_b.data(), d.n_pairs);
    put(G.offpair.data() + d.pair0, st.off_pair.data(), d.n_pairs);
    for (int pi = 0; pi < d.n_pairs; pi++) {
        const bool has_items = (st.pair_mask[pi] & 16) != 0;
        st.pair_mask[pi] &= 15;
        // S stays pristine: a sub-block nothing is ever added to keeps the zero of the upload -- without an IMU edge only
        // the 6x6 PR block of a pair is ever written, and a pair without shared landmarks is not written at all
        if (pristine && st.pair_a[pi] != st.pair_b[pi] && st.pimu_begin[pi + 1] == st.pimu_begin[pi]) st.pair_mask[pi] &= has_items ? 1 : 0;
    }
    put(G.pairmask.data() + d.pair0, st.pair_mask.data(), d.n_pairs);
    put(G.pimu_begin.data() + d.pair0 + w, st.pimu_begin.data(), (size_t)d.n_pairs + 1);
    put(G.pimu.data() + 2 * (size_t)d.pimu0, st.pimu.data(), st.pimu.size());
}

// the freshly packed tail of the incrementally copied arrays
int upload_inc_push(Handle* h, Upload& U) {
    const vba_host::BatchCursor& c = U.cur;
    for (auto& a : U.inc) {
        const size_t now = (a.id == BUF_OBSUV || a.id == BUF_OBSW || a.id == BUF_OBSKF) ? (size_t)c.obs0
                         : (a.id == BUF_PT0 || a.id == BUF_PTREF) ? (size_t)c.pt0 : (a.id == BUF_LMASK) ? (size_t)c.mask0 : (size_t)c.kf0;
        if (now > a.done) {
            if (now > a.total) return fail(h, "internal: incremental upload past the reserved size");
            HIPCHK(h, hipMemcpyAsync(reinterpret_cast<char*>(h->buf[a.id].p) + a.done * a.esz, a.base + a.done * a.esz, (now - a.done) * a.esz,
                                     hipMemcpyHostToDevice, h->up_stream));
            a.done = now;
        }
    }
    return 0;
}

// allocate and copy: what the described batch needs on the device (everything the incremental copies have not brought yet)
int upload_alloc_copy(Handle* h, Upload& U) {
    const int n = U.n;
    Staging& G = h->stg;
    vba_host::BatchTables& T = U.tab;
    const vba_host::BatchCursor& c = U.cur;
    const LaunchGeom& g = h->geom;
    const size_t kf0 = c.kf0, pt0 = c.pt0, obs0 = c.obs0, imu0 = c.imu0, pair0 = c.pair0, vec0 = c.vec0, item0 = (size_t)c.item0;
    const bool inc_on = h->up.inc_copy, idp = U.probs[0]->variant == VBA_VARIANT_PRV_IDP;
    if (h2d_vec(h, BUF_DESC, h->desc, G.s_desc)) return -1;
    if (dalloc(h, BUF_CTRL, sizeof(WinCtrl) * n)) return -1;
    if (!inc_on && (h2d(h, BUF_POSE0, G.pose) || h2d(h, BUF_VEL0, G.vel) || h2d(h, BUF_BIAS0, G.bias) || h2d(h, BUF_PT0, G.pt))) return -1;
    if (h2d(h, BUF_KFFIX, G.kffix)) return -1;
    if (dalloc(h, BUF_POSE, G.pose.size() * 8) || dalloc(h, BUF_VEL, G.vel.size() * 8) || dalloc(h, BUF_BIAS, G.bias.size() * 8)) return -1;
    if (dalloc(h, BUF_POSEBK, G.pose.size() * 8) || dalloc(h, BUF_VELBK, G.vel.size() * 8) || dalloc(h, BUF_BIASBK, G.bias.size() * 8)) return -1;
    if (dalloc(h, BUF_KFR, kf0 * 12 * 8) || dalloc(h, BUF_PT, G.pt.size() * 8) || dalloc(h, BUF_PTBK, G.pt.size() * 8)) return -1;
    if (h2d(h, BUF_PTOBS, G.ptobs)) return -1;
    if (!inc_on && (h2d(h, BUF_PTREF, G.ptref) || h2d(h, BUF_OBSKF, G.obskf) || h2d(h, BUF_LMASK, G.lmask))) return -1;
    // built on the device (vba_structure.h): record orders, keyframe segments, item lists; + the scratch of the build
    if (dalloc(h, BUF_OBSPT, obs0 * 4) || dalloc(h, BUF_SLOTPERM, obs0 * 4) || dalloc(h, BUF_PTPERM, pt0 * 4)) return -1;
    if (dalloc(h, BUF_KFSEG, (kf0 + n) * 4) || dalloc(h, BUF_REFSEG, (kf0 + n) * 4) || dalloc(h, BUF_KEYSEG, (kf0 + n) * 4)) return -1;
    if (dalloc(h, BUF_MASKQ, (size_t)c.mask0 * 8) || dalloc(h, BUF_SLOTMASK, obs0 * (size_t)g.max_mwords * 8) || dalloc(h, BUF_REFQ, pt0 * 4)) return -1;
    if (dalloc(h, BUF_SLOTO, obs0 * 4)) return -1;
    if (dalloc(h, BUF_TSLOT, obs0 * 4) || dalloc(h, BUF_KFDIR, kf0 * 32 * 8)) return -1;
    if (dalloc(h, BUF_SLOTREF, obs0 * 4) || dalloc(h, BUF_SLOTQ, obs0 * 4) || dalloc(h, BUF_RECQ, pt0 * 4) || dalloc(h, BUF_TSQ, pt0 * 8 * 4)) return -1;
    if (dalloc(h, BUF_ITEMBEG, (pair0 + n) * 4) || dalloc(h, BUF_ITEMMID, (pair0 + n) * 4) || dalloc(h, BUF_ITEMS, item0 * 8)) return -1;
    if (dalloc(h, BUF_STKEY, pt0 * 4) || dalloc(h, BUF_LMORDER, pt0 * 4) || dalloc(h, BUF_SLOTOBS, obs0 * 4) || dalloc(h, BUF_PTINV, pt0 * 4)) return -1;
    if (!inc_on && (h2d(h, BUF_OBSUV, G.uv) || h2d(h, BUF_OBSW, G.ow))) return -1;
    // (inverse-depth windows evaluate the depth of an edge where they need it, idp_edge_eval: no per-edge copy)
    if (dalloc(h, BUF_LVL, obs0) || dalloc(h, BUF_CHI2E, obs0 * 8) || dalloc(h, BUF_DEPTH, idp ? 16 : obs0 * 8)) return -1;
    if (dalloc(h, BUF_EREC, obs0 * (idp ? VBA_EREC1 : VBA_EREC) * 8) || dalloc(h, BUF_PREC, pt0 * VBA_PREC * 8)) return -1;
    if (dalloc(h, BUF_SLOT, (obs0 + pt0) * (idp ? VBA_SLOT : VBA_SLOT3) * 8)) return -1;
    if (dalloc(h, BUF_LMSD, idp ? pt0 * 16 : 16)) return -1;   // inverse depth: (sqrt(Dinv), beta) per landmark
    if (dalloc(h, BUF_OBSUVK, idp ? obs0 * 16 : 16)) return -1;   // inverse depth: the pixels in record order, beside the edge records (k_st_rec_fill)
    if (dalloc(h, BUF_CHI2F, obs0 * 8)) return -1;
    if (h2d(h, BUF_IMUI, G.imui) || h2d(h, BUF_IMUJ, G.imuj) || h2d(h, BUF_IMUMEAS, G.meas) || h2d(h, BUF_IMUINFO, G.info)) return -1;
    if (dalloc(h, BUF_IMUH, imu0 * VBA_IMUH * 8) || dalloc(h, BUF_IMUCHI, imu0 * 4 * 8) || dalloc(h, BUF_IMUJREC, imu0 * IMU_JREC * 8)) return -1;
    if (dalloc(h, BUF_S, c.S_tot * 8) || dalloc(h, BUF_VEC, vec0 * 8) || dalloc(h, BUF_BPOSE, vec0 * 2 * 8)) return -1;
    if (dalloc(h, BUF_LF, c.S_tot * 8) || dalloc(h, BUF_YV, vec0 * 8)) return -1;
    if (h2d_vec(h, BUF_TLSTEP, T.tlstep, G.s_int[0]) || h2d_vec(h, BUF_TLPAIR, T.tlpair, G.s_int[1]) || h2d_vec(h, BUF_TLPANB, T.tlpanb, G.s_int[2]) ||
        h2d_vec(h, BUF_TLPAN, T.tlpan, G.s_int[3]) || h2d_vec(h, BUF_TLKB, T.tlkb, G.s_int[4]) || h2d_vec(h, BUF_TLK, T.tlk, G.s_int[5]) ||
        h2d_vec(h, BUF_CU, T.culist, G.s_int[12]) || h2d_vec(h, BUF_CHAINTAB, T.chaintab, G.s_int[13])) return -1;
    if (dalloc(h, BUF_DVEC, vec0 * 8) || dalloc(h, BUF_WINV, (size_t)n * 1024 * 8 * (1 + (size_t)(h->up.left_looking ? g.max_nc : 0)))) return -1;
    if (dalloc(h, BUF_VARACT, vec0 * 4)) return -1;
    if (h2d(h, BUF_PAIRA, G.pair_a) || h2d(h, BUF_PAIRB, G.pair_b)) return -1;
    h->solver = U.probs[0]->solver;
    if (U.opts.pcg) {
        T.adjbeg.resize(kf0 + n, 0);
        if (h2d_vec(h, BUF_ADJBEG, T.adjbeg, G.s_int[7]) || h2d_vec(h, BUF_ADJ, T.adj, G.s_int[8])) return -1;
        if (dalloc(h, BUF_PCGV, vec0 * 5 * 8) || dalloc(h, BUF_PCGM, kf0 * 450 * 8) || dalloc(h, BUF_PCGS, (size_t)n * 8 * 8)) return -1;
    }
    if (h2d(h, BUF_PIMUBEG, G.pimu_begin) || h2d(h, BUF_PIMU, G.pimu) || h2d_vec(h, BUF_LINBLK, T.linblk, G.s_int[6])) return -1;
    T.prun0.resize(T.linblk.size() / 4 + 1, 0); T.prefbeg.resize(kf0 + n + 1, 0); T.preflist.resize(pt0 + 1, 0);
    if (h2d_vec(h, BUF_PRUN0, T.prun0, G.s_int[9]) || h2d_vec(h, BUF_PREFBEG, T.prefbeg, G.s_int[10]) || h2d_vec(h, BUF_PREFLIST, T.preflist, G.s_int[11])) return -1;
    if (h2d(h, BUF_OFFPAIR, G.offpair) || h2d(h, BUF_PAIRMASK, G.pairmask)) return -1;
    if (dalloc(h, BUF_PART, (size_t)c.part0 * 8) || dalloc(h, BUF_OUTL, obs0) || dalloc(h, BUF_OUTCHI, obs0 * 8)) return -1;
    return 0;
}

// few windows: everything the download reads lives in ONE block -- one D2H copy behind the run (do_run)
int upload_results_block(Handle* h, const Upload& U) {
    h->res_bytes = 0;
    if (!h->up.results_block) return 0;
    Staging& G = h->stg;
    const size_t obs0 = U.cur.obs0;
    const size_t sz[7] = {sizeof(WinCtrl) * (size_t)U.n, G.pose.size() * 8, G.vel.size() * 8, G.bias.size() * 8, G.pt.size() * 8, obs0, obs0 * 8};
    const int ids[7] = {BUF_CTRL, BUF_POSE, BUF_VEL, BUF_BIAS, BUF_PT, BUF_OUTL, BUF_OUTCHI};
    size_t off = 0;
    for (int i = 0; i < 7; i++) { h->res_off[i] = off; off += (std::max<size_t>(sz[i], 16) + 255) / 256 * 256; }
    if (dalloc(h, BUF_RESULTS, off)) return -1;
    HIPCHK(h, h->res_host.ensure(off));
    for (int i = 0; i < 7; i++) {
        h->buf[ids[i]].view = reinterpret_cast<char*>(h->buf[BUF_RESULTS].p) + h->res_off[i];
        h->buf[ids[i]].view_bytes = std::max<size_t>(sz[i], 16);
    }
    h->res_bytes = off;
    return 0;
}

// zero and pad -- S: zero everything once, identity on the pads (k_init_pads, behind bind_batch); the vectors; the arena copy
int upload_zero_pad(Handle* h, const Upload& U) {
    const int n = U.n;
    const size_t vec0 = U.cur.vec0;
    // (PCG reads whole keyframe-pair blocks, also the sub-blocks no factor tile covers and no Schur kernel writes: zero them once)
    if (h->up.zero_s) HIPCHK(h, hipMemsetAsync(h->buf[BUF_S].p, 0, U.cur.S_tot * 8, h->up_stream));
    for (int w = 0; w < n && !h->up.zero_s; w++) {  // only the pad rows of S must be zero (identity on their diagonal, below)
        const WinDesc& d = h->desc[w];
        if (d.order == 2) {   // pads between the parts: their COLUMNS run through tiles of the factor too -- zero the whole block once
            HIPCHK(h, hipMemsetAsync(dp<double>(h, BUF_S) + d.S0, 0, (size_t)d.nS * d.nS * 8, h->up_stream));
            continue;
        }
        for (int q = 0; q < 3; q++)
            if (d.padn[q] > 0)
                HIPCHK(h, hipMemsetAsync(dp<double>(h, BUF_S) + d.S0 + (size_t)d.pad0[q] * d.nS, 0, (size_t)d.padn[q] * d.nS * 8, h->up_stream));
    }
    HIPCHK(h, hipMemsetAsync(h->buf[BUF_VEC].p, 0, vec0 * 8, h->up_stream));
    HIPCHK(h, hipMemsetAsync(h->buf[BUF_YV].p, 0, vec0 * 8, h->up_stream));
    HIPCHK(h, hipMemsetAsync(h->buf[BUF_BPOSE].p, 0, vec0 * 16, h->up_stream));
    return h2d_flush(h);
}

// the device pointers of the uploaded batch
int bind_batch(Handle* h, int n, bool idp) {
    Batch& B = h->B;
    B.desc = dp<WinDesc>(h, BUF_DESC); B.ctrl = dp<WinCtrl>(h, BUF_CTRL); B.n_win = n;
    B.pose = dp<double>(h, BUF_POSE); B.vel = dp<double>(h, BUF_VEL); B.bias = dp<double>(h, BUF_BIAS); B.kfR = dp<double>(h, BUF_KFR);
    B.pose0 = dp<double>(h, BUF_POSE0); B.vel0 = dp<double>(h, BUF_VEL0); B.bias0 = dp<double>(h, BUF_BIAS0);
    B.pose_bk = dp<double>(h, BUF_POSEBK); B.vel_bk = dp<double>(h, BUF_VELBK); B.bias_bk = dp<double>(h, BUF_BIASBK);
    B.pt = dp<double>(h, BUF_PT); B.pt0 = dp<double>(h, BUF_PT0); B.pt_bk = dp<double>(h, BUF_PTBK);
    B.pt_ref = dp<int>(h, BUF_PTREF); B.pt_obs_begin = dp<int>(h, BUF_PTOBS);
    B.obs_kf = dp<int>(h, BUF_OBSKF); B.obs_pt = dp<int>(h, BUF_OBSPT);
    B.obs_uv = dp<double>(h, BUF_OBSUV); B.obs_w = dp<double>(h, BUF_OBSW);
    B.obs_uvk = idp ? dp<double>(h, BUF_OBSUVK) : nullptr;
    B.lvl = dp<unsigned char>(h, BUF_LVL); B.chi2_e = dp<double>(h, BUF_CHI2E); B.depth_e = dp<double>(h, BUF_DEPTH);
    B.chi2_f = idp ? nullptr : dp<double>(h, BUF_CHI2F);
    B.erec = dp<double>(h, BUF_EREC); B.prec = dp<double>(h, BUF_PREC); B.slot = dp<double>(h, BUF_SLOT); B.lm_sd = dp<double2>(h, BUF_LMSD); B.kf_fix = dp<unsigned char>(h, BUF_KFFIX);
    B.imu_i = dp<int>(h, BUF_IMUI); B.imu_j = dp<int>(h, BUF_IMUJ);
    B.imu_meas = dp<double>(h, BUF_IMUMEAS); B.imu_info = dp<double>(h, BUF_IMUINFO);
    B.imuH = dp<double>(h, BUF_IMUH); B.imu_chi = dp<double>(h, BUF_IMUCHI); B.imu_jrec = dp<double>(h, BUF_IMUJREC);
    B.S = dp<double>(h, BUF_S); B.vec = dp<double>(h, BUF_VEC); B.bpose = dp<double>(h, BUF_BPOSE);
    B.Lf = dp<double>(h, BUF_LF); B.yv = dp<double>(h, BUF_YV);
    B.l_packed = h->up.left_looking;
    B.tl_step_begin = dp<int>(h, BUF_TLSTEP); B.tl_pairs = dp<int>(h, BUF_TLPAIR);
    B.tl_pan_begin = dp<int>(h, BUF_TLPANB); B.tl_pan = dp<int>(h, BUF_TLPAN);
    B.tl_kl_begin = dp<int>(h, BUF_TLKB); B.tl_kl = dp<int>(h, BUF_TLK); B.tl_cu = dp<int>(h, BUF_CU); B.tl_ct = dp<int>(h, BUF_CHAINTAB);
    B.dvec = dp<double>(h, BUF_DVEC); B.winv = dp<double>(h, BUF_WINV); B.w_total = n; B.w_stride = h->geom.max_nc;
    B.slot_perm = dp<int>(h, BUF_SLOTPERM); B.pt_perm = dp<int>(h, BUF_PTPERM);
    B.var_act = dp<int>(h, BUF_VARACT);
    B.pair_a = dp<int>(h, BUF_PAIRA); B.pair_b = dp<int>(h, BUF_PAIRB);
    B.item_begin = dp<int>(h, BUF_ITEMBEG); B.items = dp<int>(h, BUF_ITEMS); B.item_mid = dp<int>(h, BUF_ITEMMID);
    B.kf_dir = dp<double>(h, BUF_KFDIR); B.slot_lm = dp<int>(h, BUF_SLOTOBS); B.slot_o = dp<int>(h, BUF_SLOTO); B.rec_lm = dp<int>(h, BUF_PTINV);
    B.adj_begin = dp<int>(h, BUF_ADJBEG); B.adj = dp<int>(h, BUF_ADJ); B.pcg_v = dp<double>(h, BUF_PCGV); B.pcg_m = dp<double>(h, BUF_PCGM); B.pcg_s = dp<double>(h, BUF_PCGS);
    B.lmask = dp<unsigned long long>(h, BUF_LMASK); B.kf_seg = dp<int>(h, BUF_KFSEG); B.ref_seg = dp<int>(h, BUF_REFSEG);
    B.pimu_begin = dp<int>(h, BUF_PIMUBEG); B.pimu = dp<int>(h, BUF_PIMU);
    B.lin_blk = dp<int>(h, BUF_LINBLK);
    B.prun0 = dp<int>(h, BUF_PRUN0); B.pref_begin = dp<int>(h, BUF_PREFBEG); B.pref_list = dp<int>(h, BUF_PREFLIST);
    B.off_pair = dp<int>(h, BUF_OFFPAIR); B.pair_mask = dp<int>(h, BUF_PAIRMASK);
    B.part = dp<double>(h, BUF_PART);
    B.stop_host_word = h->stop_dev;
    B.alive_cnt = h->stop_dev + 64;
    if (dalloc(h, BUF_ALIVE, 14 * 1024 * sizeof(int))) return -1;
    B.alive_dev = dp<int>(h, BUF_ALIVE);
    B.stop_word = stop_word_of(h, B);
    B.out_outlier = dp<unsigned char>(h, BUF_OUTL); B.out_chi2 = dp<double>(h, BUF_OUTCHI);
    if (dalloc(h, BUF_DBG, 4096)) return -1;
    B.dbg = dp<double>(h, BUF_DBG);
    return 0;
}

// the device half of the structure build (vba_structure.h)
int enqueue_structure_build(Handle* h, const Upload& U) {
    const int n = U.n;
    const Batch& B = h->B;
    const LaunchGeom& g = h->geom;
    StBuild T;
    T.obs_pt = dp<int>(h, BUF_OBSPT); T.slot_perm = dp<int>(h, BUF_SLOTPERM); T.pt_perm = dp<int>(h, BUF_PTPERM);
    T.kf_seg = dp<int>(h, BUF_KFSEG); T.ref_seg = dp<int>(h, BUF_REFSEG);
    T.item_begin = dp<int>(h, BUF_ITEMBEG); T.item_mid = dp<int>(h, BUF_ITEMMID); T.items = dp<int>(h, BUF_ITEMS);
    T.st_key = dp<int>(h, BUF_STKEY); T.lm_order = dp<int>(h, BUF_LMORDER); T.slot_obs = dp<int>(h, BUF_SLOTOBS); T.pt_inv = dp<int>(h, BUF_PTINV);
    const size_t sh_order = 3 * ((size_t)g.max_kf + 1) * sizeof(int), sh_row = 2 * (size_t)std::max(1, g.max_free) * sizeof(int);
    if (sh_order > 60000 || sh_row > 60000) return fail(h, "window with too many keyframes for the structure build");
    T.key_seg = dp<int>(h, BUF_KEYSEG); T.tslot = dp<int>(h, BUF_TSLOT);
    T.mask_q = dp<unsigned long long>(h, BUF_MASKQ); T.slot_mask = dp<unsigned long long>(h, BUF_SLOTMASK); T.ref_q = dp<int>(h, BUF_REFQ);
    T.smw = g.max_mwords;
    T.row_lds = h->up.row_lds;
    T.slot_o = dp<int>(h, BUF_SLOTO);
    T.obs_uvk = const_cast<double*>(B.obs_uvk);
    T.slot_ref = dp<int>(h, BUF_SLOTREF); T.slot_q = dp<int>(h, BUF_SLOTQ); T.rec_q = dp<int>(h, BUF_RECQ); T.tsq = dp<int>(h, BUF_TSQ);
    VBA_LAUNCH(k_st_hist, dim3(n), dim3(h->up.hist_block), sh_order, h->up_stream, B, T);
    {
        const int max_chunks = std::max(1, g.max_pt_blk);   // 64-landmark blocks of the largest window
        if (dalloc(h, BUF_RECCNT, (size_t)U.cur.kf0 * max_chunks * 2 * 4)) return -1;
        T.rec_cnt = dp<int>(h, BUF_RECCNT);
        VBA_LAUNCH(k_st_lm_count, dim3(max_chunks, n), dim3(64), 0, h->up_stream, B, T, max_chunks);
        VBA_LAUNCH(k_st_rec_scan, dim3(n), dim3(256), 0, h->up_stream, B, T, max_chunks);
        VBA_LAUNCH(k_st_lm_fill, dim3(max_chunks, n), dim3(64), 0, h->up_stream, B, T, max_chunks);
        VBA_LAUNCH(k_st_rec_count, dim3(max_chunks, n), dim3(64), 0, h->up_stream, B, T, max_chunks);
        VBA_LAUNCH(k_st_rec_scan, dim3(n), dim3(256), 0, h->up_stream, B, T, max_chunks);
        VBA_LAUNCH(k_st_rec_fill, dim3(max_chunks, n), dim3(64), 0, h->up_stream, B, T, max_chunks);
    }
    VBA_LAUNCH(k_st_count, dim3(g.max_free, n), dim3(64), sh_row, h->up_stream, B, T, g.max_free);
    VBA_LAUNCH(k_st_scan, dim3(n), dim3(256), 0, h->up_stream, B, T);
    VBA_LAUNCH(k_st_fill, dim3(g.max_free, n), dim3(64), sh_row, h->up_stream, B, T, g.max_free);
    HIPCHK(h, hipGetLastError());
    return 0;
}

int do_upload(Handle* h, int n, vba_problem* const* probs, bool defer_sync = false) {
    const bool timing = vba_host::process_knobs().timing;
    const double t_begin = now_ms();
    if (n <= 0) return fail(h, "empty batch");
    Upload U;
    U.n = n;
    U.probs = probs;
    if (upload_begin(h, U)) return -1;
    Staging& G = h->stg;
    LaunchGeom& g = h->geom;
    // Per chunk of windows: (1) the per-window structure on a pool of host threads, (2) descriptors and offsets in window order on
    // this thread, (3) the concatenated arrays grown once, (4) the pool again copies every window's arrays to its offsets.
    const int chunk = 8 * U.n_threads;
    for (int chunk0 = 0; chunk0 < n; chunk0 += chunk) {
        const int cn = std::min(chunk, n - chunk0);
        if (upload_structures(h, U, chunk0, cn) || upload_describe(h, U, chunk0, cn) || upload_grow_staging(h, U, chunk0 + cn)) return -1;
        host_parallel_for(h, cn, std::min(U.n_threads, cn), [&](int q) { pack_window(G, probs[chunk0 + q], h->desc[chunk0 + q], U.sts[q], h->up.left_looking); });
        if (h->up.inc_copy && upload_inc_push(h, U)) return -1;
    }
    if (h->up.inc_copy && (G.uv.data() != reinterpret_cast<const double*>(U.inc[0].base) || G.pt.data() != reinterpret_cast<const double*>(U.inc[3].base)))
        return fail(h, "internal: the upload staging moved under an incremental copy");
    h->algo = probs[0]->algo;
    h->variant = probs[0]->variant;
    if (g.chain_lds > 40 * 1024 || g.max_nc > 256) {   // (256: CHAIN_MAX_NC)   // (a window whose tile tables do not fit beside the kernel's 53 KB of tiles: one launch per column)
        for (auto& d : h->desc) { d.nc = 0; d.n_cu = 0; }
        g.min_nc = g.max_nc = g.max_cu = 0;
    }
    if (!U.opts.pcg) {   // the back-substitution keeps x, its solve blocks and the window's tile lists in LDS (160 KiB per workgroup)
        const size_t shm = ((size_t)g.max_nS + 2 * TRSV_P_DW * 32 + 2 * 32 * 65 + 32) * sizeof(double) + ((size_t)g.max_pan + g.max_nb + 2) * sizeof(int);
        if (shm > 160 * 1024) return fail(h, "window too large for the direct solver (back-substitution workspace > 160 KiB of LDS): use VBA_SOLVER_PCG");
    }
    const double t_pack = now_ms();
    if (upload_alloc_copy(h, U) || upload_results_block(h, U) || upload_zero_pad(h, U)) return -1;
    if (bind_batch(h, n, probs[0]->variant == VBA_VARIANT_PRV_IDP)) return -1;
    static_assert(VBA_NB <= 64, "k_init_pads covers the pads with one wave");
    VBA_LAUNCH(k_init_pads, dim3(n), dim3(64), 0, h->up_stream, h->B);   // pads of S: identity on the padded diagonal, written once (the solve never touches them)
    if (enqueue_structure_build(h, U)) return -1;
    const double t_enq = now_ms();
    // vba_solve (one call: upload, run, download) does not come back to the host here: the run stream waits for the upload stream
    // on the device (an event), and the run's kernels queue up behind the structure build instead of behind a host round trip
    h->up_pending = false;
    if (defer_sync && h->up_done) {
        HIPCHK(h, hipEventRecord(h->up_done, h->up_stream));
        h->up_pending = true;
    } else
        HIPCHK(h, hipStreamSynchronize(h->up_stream));
    if (timing) fprintf(stderr, "[vba] chain columns: min %d max %d, update tiles %d, rows %d, ll %d\n", g.min_nc, g.max_nc, g.max_cu, g.max_chain_rows, h->up.left_looking);
    if (timing) fprintf(stderr, "[vba] %p t=%.1f upload %d windows: total %.3f ms (structure %.3f, pack %.3f, alloc+H2D enqueue %.3f, sync %.3f)\n", (void*)h, now_ms(), n,
                        now_ms() - t_begin, U.t_struct, t_pack - t_begin - U.t_struct, t_enq - t_pack, now_ms() - t_enq);
    h->uploaded = true;
    h->ran = false;
    h->dl_prefetched = false;
    return 0;
}

}  // namespace
