// vba_host_batch.h -- host side of the library, part 4: handle creation (a handle of its own, a lane, an arena), vba_solve,
// vba_batch_solve (chunks of a batch on lanes) and the asynchronous tickets of vba_batch_submit.
#pragma once

namespace {

// vba_batch_submit (defined with it, below): the synchronous entry points refuse while a ticket is submitted and not retired
int async_busy(Handle* h);
// vba_destroy: the pending tickets finish (their results land in the callers' arrays), the workers are joined, the arenas freed
void async_shutdown(Handle* h);

// parent == nullptr: a handle of its own (four streams, created NOW, before anything ran: created after a first solve they do
// not run concurrently with it -- measured: 64 windows in 4 groups 16.4 ms instead of 11.3 ms when a one-window solve came
// first; the runtime binds streams to its hardware queues when they are created).
// parent != nullptr: a lane of vba_batch_solve.  It owns device buffers, pinned staging and control words, but SHARES the
// parent's four streams, one role each: [0] run, [1] run (second window group), [2] upload (H2D + structure build), [3]
// download (D2H).  The runtime multiplexes streams onto four hardware queues; with streams of their own the lanes' uploads
// landed in the queue of another lane's solve and stalled it behind their transfers (head-of-line blocking: 512 windows
// solved in 70 ms instead of 52).  Only one lane solves at a time (run token), so the run streams are never contended.
int make_handle(int device, Handle* parent, Handle** out) {
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) return -2;  // no CPU fallback
    Handle* h = new Handle();
    h->device = device;
    if (hipSetDevice(device) != hipSuccess) { delete h; return -3; }
    if (parent) {
        if (parent->xstreams.size() < 3) { delete h; return -3; }
        h->owns_streams = false;
        h->is_lane = true;
        h->stream = parent->stream;
        h->xstreams.push_back(parent->xstreams[0]);
        h->up_stream = parent->xstreams[1];
        h->dl_stream = parent->xstreams[2];
    } else {
        if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) { delete h; return -3; }
        for (int i = 0; i < 3; i++) {
            hipStream_t st;
            if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) break;
            h->xstreams.push_back(st);
        }
        h->up_stream = h->dl_stream = h->stream;
    }
    void* hp = nullptr;
    if (hipHostMalloc(&hp, 8192, hipHostMallocMapped) != hipSuccess) { delete h; return -4; }   // [0,1024) run control words, [1024,2048) PCG rings
    memset(hp, 0, 8192);
    h->stop_host = reinterpret_cast<volatile int*>(hp);
    *h->stop_host = 0;
    void* dpw = nullptr;
    if (hipHostGetDevicePointer(&dpw, hp, 0) != hipSuccess) { delete h; return -5; }
    h->stop_dev = reinterpret_cast<int*>(dpw);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k_lin2), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)LIN2_LDS);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k_lin2_imu), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)LIN2_LDS);
    // the back-substitution keeps x (nS doubles) in LDS: maps of more than ~5 600 pose dofs need more than the default 64 KiB
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k_trsv), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k_trsv_p), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    // the claim table of k_search_proj (VBA_SP_MAX_KEYS int32) beside its static LDS
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k_search_proj), hipFuncAttributeMaxDynamicSharedMemorySize, 4 * (VBA_SP_MAX_KEYS + 1));
    // the claim table of k_search_bow (VBA_SB_MAX_KEYS int32): its only LDS
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k_search_bow), hipFuncAttributeMaxDynamicSharedMemorySize, 4 * (VBA_SB_MAX_KEYS + 1));
    // the list heads of k_search_init (VBA_SI_MAX_KEYS int32) beside its static LDS
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k_search_init), hipFuncAttributeMaxDynamicSharedMemorySize, 4 * (VBA_SI_MAX_KEYS + 1));
    (void)hipEventCreateWithFlags(&h->up_done, hipEventDisableTiming);
    memset(&h->prof, 0, sizeof h->prof);
    *out = h;
    return 0;
}

int solve_one(void* handle, vba_problem* inout, vba_result* out, StopRef stop_flag) {
    Handle* h = reinterpret_cast<Handle*>(handle);
    if (!h || !inout || !out) return -1;
    if (async_busy(h)) return -1;
    if (stop_flag.set()) {  // src/Optimizer.cpp:453-455: return before anything is built
        out->status = VBA_ABORTED_BEFORE;
        out->its_done[0] = out->its_done[1] = 0;
        out->n_outliers = 0; out->n_trace = 0; out->lin_iterations = 0;
        out->chi2_vis = out->chi2_prv = out->chi2_bias = 0;
        return 0;
    }
    vba_problem* ps[1] = {inout};
    vba_result* rs[1] = {out};
    if (do_upload(h, 1, ps, true)) return -1;
    if (do_run(h, stop_flag)) return -1;
    return do_download(h, 1, ps, rs);
}

// Fresh windows in, solved windows out: the batch is cut into chunks and several chunks are in flight at once, each on its
// own lane (a sub-handle with its own streams, device buffers and pinned staging), so that the host-side packing, the H2D
// transfer and the structure build of chunk k+1 and the D2H + scatter of chunk k-1 run while chunk k is being solved.
// Windows are independent (one function-local optimiser per call in the reference, src/Optimizer.cpp:130).  A chunk runs the
// kernels a batch of its size runs (the choice depends on the window count: thresholds 8 / 64 / 256), so chunks of the
// default size give bit for bit what one big upload + run + download gives; across a threshold the sums run in another
// fixed order and the results agree to rounding.
int batch_solve(void* handle, int32_t n, vba_problem* const* inout, vba_result* const* out, StopRef stop_flag) {
    Handle* h = reinterpret_cast<Handle*>(handle);
    if (!h || async_busy(h)) return -1;
    if (n <= 0 || !inout) return fail(h, "vba_batch_solve: bad arguments");
    // chunk boundaries and lanes: vba_host_plan.h (a ramp at the start, then equal chunks; no chunk below 256 windows when the batch has that many)
    const vba_host::Knobs K = vba_host::current_knobs();
    const std::vector<int> cbeg = vba_host::chunk_bounds(n, vba_host::chunk_max_of(h->ov, K), !K.no_ramp, K.chunks);
    const int n_lanes = vba_host::lanes_of(h->ov, K, (int)cbeg.size() - 1);
    if (cbeg.size() == 2) {
        if (do_upload(h, n, inout) || do_run(h, stop_flag)) return -1;
        return do_download(h, n, inout, out);
    }
    while ((int)h->lanes.size() < n_lanes) {
        Handle* l = nullptr;
        if (make_handle(h->device, h, &l) != 0) return fail(h, "vba_batch_solve: could not create a lane");
        l->ov.path = h->ov.path;   // (the path overrides only: a lane takes VBA_LANE_STREAMS, not the parent's streams)
        h->lanes.push_back(l);
    }
    const int n_chunks2 = (int)cbeg.size() - 1;
    std::atomic<int> next(0), bad(0);
    // Lanes that start together stay in step (all pack, then all solve, then all scatter: the GPU idles while the hosts pack).
    // A run token breaks the symmetry: only `run_slots` lanes may be inside the solve at a time, the others pack / transfer /
    // build the structure of their next chunk or scatter their last one meanwhile.
    int run_free = std::max(1, std::min(K.run_slots, n_lanes));
    std::mutex run_mu;
    std::condition_variable run_cv;
    auto run_gated = [&](Handle* lane) -> int {
        {
            std::unique_lock<std::mutex> lk(run_mu);
            run_cv.wait(lk, [&] { return run_free > 0; });
            run_free--;
        }
        const int rc = do_run(lane, stop_flag);
        {
            std::lock_guard<std::mutex> lk(run_mu);
            run_free++;
        }
        run_cv.notify_one();
        return rc;
    };
    const bool timing = K.timing;
    const double t_call = now_ms();
    int up_turn = 0;
    std::mutex up_mu;
    std::condition_variable up_cv;
    auto work = [&](Handle* lane) {
        for (int c = next.fetch_add(1); c < n_chunks2 && !bad.load(); c = next.fetch_add(1)) {
            const int w0 = cbeg[c], cn = cbeg[c + 1] - w0;
            if (cn <= 0) {
                { std::unique_lock<std::mutex> lk(up_mu); up_cv.wait(lk, [&] { return up_turn == c || bad.load(); }); up_turn = c + 1; }
                up_cv.notify_all();
                continue;
            }
            {   // uploads go one at a time, in chunk order: the first chunk gets every host thread and the whole link (lanes that
                // start together share them and the device waits for the slower of two half-speed uploads), and a third lane
                // can have chunk c+1 on the device before chunk c's solve ends
                std::unique_lock<std::mutex> lk(up_mu);
                up_cv.wait(lk, [&] { return up_turn == c || bad.load(); });
            }
            const double t0 = now_ms();
            int rc = bad.load() ? -1 : do_upload(lane, cn, inout + w0);
            {
                std::lock_guard<std::mutex> lk(up_mu);
                up_turn = c + 1;
            }
            up_cv.notify_all();
            const double t1 = now_ms();
            if (!rc) rc = run_gated(lane);
            const double t2 = now_ms();
            if (!rc) rc = do_download(lane, cn, inout + w0, out ? out + w0 : nullptr);
            if (timing) fprintf(stderr, "[vba_batch_solve] chunk %d (%d windows): upload %.1f..%.1f  run ..%.1f  download ..%.1f ms\n", c, cn, t0 - t_call, t1 - t_call, t2 - t_call, now_ms() - t_call);
            if (rc) {
                {   // the message and `bad` change together, under the mutex the waiting lanes evaluate their predicate under: the first
                    // failing lane writes the message (two lanes failing together cannot both), and a lane that has just found
                    // `up_turn == c || bad` false cannot miss this wake-up
                    std::lock_guard<std::mutex> lk(up_mu);
                    if (!bad.load()) h->err = "vba_batch_solve, windows " + std::to_string(w0) + ".." + std::to_string(w0 + cn - 1) + ": " + lane->err;
                    bad.store(1);
                }
                up_cv.notify_all();   // lanes waiting for their upload turn see `bad`
                return;
            }
        }
    };
    std::vector<std::thread> pool;
    for (int l = 1; l < n_lanes; l++) pool.emplace_back(work, h->lanes[l]);
    work(h->lanes[0]);
    for (auto& t : pool) t.join();
    return bad.load() ? -1 : 0;
}

// ---- asynchronous batches: vba_batch_submit / vba_batch_poll / vba_batch_wait -------------------------------------------------
// A caller with one batch after another hands over batch k+1 while batch k solves.  Every ticket is ONE upload + run + download
// on an arena -- a lane (make_handle) that owns its device buffers and pinned staging and shares the parent's four streams -- so
// it gets bit for bit what vba_batch_upload + run + download of that batch gives (the kernel choice depends on the number of
// windows in a run: thresholds 8 / 64 / 256; a chunked run would change it).  One persistent worker per arena, `depth` of them,
// started at the first submit, takes the next ticket; uploads, runs and downloads each go one at a time in ticket order (the
// turns of batch_solve), so the packing, H2D copies and structure build of ticket k+1 and the D2H copies and scatter of ticket
// k-1 overlap the solve of ticket k.  A worker writes its arena's `err` and its ticket only; the parent's `err` is written on
// the caller's thread (submit / poll / wait).
struct AsyncTicket {
    int64_t id = 0;
    std::vector<vba_problem*> inout;   // the caller's pointer arrays, copied at submit
    std::vector<vba_result*> out;      // empty: out == NULL
    StopRef stop;
    bool done = false;                 // rc, err, done: written by the worker under AsyncState::mu
    int rc = 0;
    std::string err;                   // the arena's message of the stage that failed
    double t[6] = {0, 0, 0, 0, 0, 0};  // upload, run, download: start and end, ms from the first submit (VBA_TIMING)
};
struct AsyncState {
    std::mutex mu;
    std::condition_variable cv;        // every change of the fields below: notify_all
    std::map<int64_t, std::shared_ptr<AsyncTicket>> tickets;   // submitted, not retired (caller's thread only)
    std::deque<std::shared_ptr<AsyncTicket>> queue;            // submitted, not taken by a worker yet
    int64_t next_id = 1;
    int64_t up_turn = 1, run_turn = 1, dl_turn = 1;            // the ticket whose upload / run / download may start
    bool hold = false;                 // vba_debug_async_hold: no upload starts
    bool quit = false;                 // workers leave once the queue is empty
    int64_t dead_at = 0;               // > 0: the ticket whose HIP error fails every later ticket with dead_msg
    std::string dead_msg;
    std::vector<Handle*> arenas;       // arenas[i] is worked by workers[i]
    std::vector<std::thread> workers;
    HostBudget budget;                 // vba_host_threads(), shared by the packing and scatter pools of the arenas
    double t0 = 0;                     // first submit (timeline)
};

AsyncState& async_state(Handle* h) {
    if (!h->as) {
        h->as = new AsyncState();
        h->as->t0 = now_ms();
        h->as->budget.free = host_threads();
    }
    return *h->as;
}

void async_worker(Handle* h, Handle* arena) {
    const bool timing = vba_host::process_knobs().timing;
    AsyncState& A = *h->as;
    (void)hipSetDevice(h->device);
    for (;;) {
        std::shared_ptr<AsyncTicket> t;
        {
            std::unique_lock<std::mutex> lk(A.mu);
            A.cv.wait(lk, [&] { return A.quit || !A.queue.empty(); });
            if (A.queue.empty()) return;
            t = A.queue.front();
            A.queue.pop_front();
        }
        const int64_t k = t->id;
        const int n = (int)t->inout.size();
        vba_problem* const* P = t->inout.data();
        vba_result* const* R = t->out.empty() ? nullptr : t->out.data();
        int rc = 0;
        bool fatal = false;
        std::string msg;
        // one stage: wait for its turn, run it unless the ticket failed already or a HIP error of an earlier ticket forbids GPU work,
        // pass the turn on -- a failed ticket passes it too, so that later tickets are not deadlocked.  A HIP error (every failure
        // of a run or a download, a failed HIP call of an upload) fails this ticket and every later one; a rejected window only this one.
        auto stage = [&](int64_t AsyncState::*turn, int slot, bool always_fatal, const std::function<int()>& body) {
            {
                std::unique_lock<std::mutex> lk(A.mu);
                A.cv.wait(lk, [&] { return A.*turn == k && !(turn == &AsyncState::up_turn && A.hold); });
                if (!rc && A.dead_at && A.dead_at < k) { rc = -1; msg = A.dead_msg; }
            }
            if (!rc) {
                arena->hip_failed = false;
                t->t[slot] = now_ms() - A.t0;
                rc = body();
                t->t[slot + 1] = now_ms() - A.t0;
                if (rc) { msg = arena->err; fatal = always_fatal || arena->hip_failed; }
            }
            {
                std::lock_guard<std::mutex> lk(A.mu);
                if (fatal && !A.dead_at) { A.dead_at = k; A.dead_msg = msg; }
                A.*turn = k + 1;
            }
            A.cv.notify_all();
        };
        stage(&AsyncState::up_turn, 0, false, [&] { return do_upload(arena, n, P); });
        stage(&AsyncState::run_turn, 2, true, [&] { return do_run(arena, t->stop); });
        stage(&AsyncState::dl_turn, 4, true, [&] { return do_download(arena, n, P, R); });
        if (timing) fprintf(stderr, "[vba_batch_submit] ticket %lld (%d windows): upload %.1f..%.1f  run %.1f..%.1f  download %.1f..%.1f ms%s\n",
                            (long long)k, n, t->t[0], t->t[1], t->t[2], t->t[3], t->t[4], t->t[5], rc ? "  FAILED" : "");
        {
            std::lock_guard<std::mutex> lk(A.mu);
            t->rc = rc;
            t->err = msg;
            t->done = true;
        }
        A.cv.notify_all();
    }
}

int async_busy(Handle* h) {
    if (h->as && !h->as->tickets.empty()) return fail(h, "asynchronous batches pending: wait for them first");
    return 0;
}

void async_stop_workers(AsyncState& A) {
    {
        std::lock_guard<std::mutex> lk(A.mu);
        A.hold = false;
        A.quit = true;
    }
    A.cv.notify_all();
    for (auto& w : A.workers) w.join();   // (a worker leaves once the queue is empty: every ticket it took has finished)
    A.workers.clear();
    A.quit = false;
}

void async_shutdown(Handle* h) {
    AsyncState* A = h->as;
    async_stop_workers(*A);
    for (Handle* a : A->arenas) (void)vba_destroy(a);
    delete A;
    h->as = nullptr;
}

int submit(Handle* h, int32_t n, vba_problem* const* inout, vba_result* const* out, StopRef stop, int64_t* ticket) {
    if (!h) return -1;
    if (!ticket || n <= 0 || !inout) return fail(h, "vba_batch_submit: bad arguments");
    *ticket = 0;
    AsyncState& A = async_state(h);
    if (A.workers.empty()) {
        while ((int)A.arenas.size() < h->async_depth) {
            Handle* a = nullptr;
            if (make_handle(h->device, h, &a) != 0) return fail(h, "vba_batch_submit: could not create an arena");
            a->ov.path = h->ov.path;   // (the path overrides of the parent, as the lanes of vba_batch_solve take them)
            a->budget = &A.budget;
            A.arenas.push_back(a);
        }
        for (int i = 0; i < h->async_depth; i++) A.workers.emplace_back(async_worker, h, A.arenas[i]);
    }
    auto t = std::make_shared<AsyncTicket>();
    t->id = A.next_id++;
    t->inout.assign(inout, inout + n);
    if (out) t->out.assign(out, out + n);
    t->stop = stop;
    A.tickets[t->id] = t;
    {
        std::lock_guard<std::mutex> lk(A.mu);
        A.queue.push_back(t);
    }
    A.cv.notify_all();
    *ticket = t->id;
    return 0;
}

}  // namespace
