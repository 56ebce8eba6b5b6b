// Sanitizer harness of the description half of an upload (mc_slam_amd/csrc/vba_host_layout.h): plain C++, built by
// tests/test_host_layout.py with g++ -fsanitize=address,undefined.
//   host_layout_check [@field=value]... <file.vbap> ... [-- <file.vbap> ...]
// Every "--" starts another batch; the batches are described one after the other with ONE LaunchGeom, reset per batch by the
// assignment an upload resets it with.  "@field=value" in front of a file overrides that field of the loaded problem (the
// reader refuses some of the values a caller can hand to the library).  Per batch: one line "win ..." per window -- or
// "refused <window> <message>", which ends the batch -- and one line "end ..." with the final cursor, table sizes and geometry.
#include "../mc_slam_amd/csrc/vba_host_layout.h"
#include "../mc_slam_amd/csrc/vba_problem_io.h"

#include <cstring>
#include <map>
#include <memory>
#include <string>

using namespace vba_host;

static void print_list(const char* key, const std::vector<int>& v) {
    printf(" %s ", key);
    if (v.empty()) printf("-");
    for (size_t i = 0; i < v.size(); i++) printf(i ? ",%d" : "%d", v[i]);
}

static bool override_field(vba_problem* P, const std::string& key, int v) {
    const std::map<std::string, int32_t*> f = {{"variant", &P->variant}, {"algo", &P->algo}, {"solver", &P->solver}, {"protocol", &P->protocol},
        {"its_stage1", &P->its_stage1}, {"its_stage2", &P->its_stage2}, {"n_kf_free", &P->n_kf_free}, {"n_pt", &P->n_pt}, {"n_obs", &P->n_obs}, {"n_imu", &P->n_imu}};
    if (key == "imu_null") { P->imu_meas = nullptr; return true; }
    auto it = f.find(key);
    if (it == f.end()) return false;
    *it->second = v;
    return true;
}

static void describe_batch(const std::vector<vba_problem*>& probs, LaunchGeom& geom) {
    geom = LaunchGeom();
    BatchCursor cur;
    BatchTables tab;
    DescribeOpts opts;
    opts.pcg = probs[0]->solver == VBA_SOLVER_PCG;
    opts.chain_on = true;
    for (size_t w = 0; w < probs.size(); w++) {
        const vba_problem* P = probs[w];
        Structure st;
        std::string err;
        WinDesc d;
        std::memset(&d, 0, sizeof d);
        const char* msg = check_window(P, probs[0]);
        if (!msg && !window_sizes_ok(P)) msg = "internal: check_window passed what window_sizes_ok refuses";
        if (!msg && build_structure(P, st, err, true)) msg = err.c_str();
        if (!msg) msg = describe_window(P, st, opts, cur, geom, tab, d);
        if (msg) { printf("refused %zu %s\n", w, msg); return; }
        printf("win %d variant %d n_kf %d n_free %d n_pt %d n_obs %d n_imu %d pdim %d np %d nS %d nb %d order %d its0 %d its1 %d", d.win, d.variant, d.n_kf, d.n_free,
               d.n_pt, d.n_obs, d.n_imu, d.pdim, d.np, d.nS, d.nb, d.order, d.its[0], d.its[1]);
        printf(" kf0 %d pt0 %d obs0 %d imu0 %d pair0 %d n_pairs %d pimu0 %d vec0 %d part0 %d item0 %d mask0 %lld mwords %d S0 %lld", d.kf0, d.pt0, d.obs0, d.imu0,
               d.pair0, d.n_pairs, d.pimu0, d.vec0, d.part0, d.item0, d.mask0, d.mwords, d.S0);
        printf(" n_part_lin %d n_part_pt %d lin_runs %d nc %d nc_split %d n_cu %d pan %zu tiles %zu", d.n_part_lin, d.n_part_pt, d.lin_runs, d.nc, d.nc_split, d.n_cu,
               st.pan.size(), st.tpairs.size());
        std::vector<int> vd, vh;
        for (int a = 0; a < d.n_free; a++)
            for (int r = 0; r < d.pdim; r++) { vd.push_back(vpos(d, a, r)); vh.push_back(vpos_host(d.order, d.pdim, d.n_free, a, r)); }
        print_list("vpos", vd);
        print_list("vpos_host", vh);
        print_list("pad0", std::vector<int>(d.pad0, d.pad0 + 3));
        print_list("padn", std::vector<int>(d.padn, d.padn + 3));
        printf("\n");
    }
    printf("end windows %d kf0 %d pt0 %d obs0 %d imu0 %d pair0 %d pimu0 %d vec0 %d part0 %d item0 %lld mask0 %lld S_tot %zu", cur.win, cur.kf0, cur.pt0, cur.obs0,
           cur.imu0, cur.pair0, cur.pimu0, cur.vec0, cur.part0, cur.item0, cur.mask0, cur.S_tot);
    printf(" tlstep %zu tlpanb %zu tlpair %zu tlpan %zu linblk %zu culist %zu chaintab %zu", tab.tlstep.size(), tab.tlpanb.size(), tab.tlpair.size(), tab.tlpan.size(),
           tab.linblk.size(), tab.culist.size(), tab.chaintab.size());
    printf(" max_pt_blk %d max_imu %d max_pairs %d max_nb %d max_obs_blk %d max_kf_blk %d max_ns_blk %d max_nS %d max_its0 %d max_its1 %d max_free %d max_lin_blk %d"
           " max_quads %d max_offp %d max_pan %d max_kf %d max_mwords %d chain_lds %zu min_nc %d max_nc %d max_cu %d max_chain_rows %d max_split %d step_grid %zu pan_grid %zu"
           " tile_updates %.0f any_lin_fallback %d\n", geom.max_pt_blk, geom.max_imu, geom.max_pairs, geom.max_nb, geom.max_obs_blk, geom.max_kf_blk, geom.max_ns_blk,
           geom.max_nS, geom.max_its[0], geom.max_its[1], geom.max_free, geom.max_lin_blk, geom.max_quads, geom.max_offp, geom.max_pan, geom.max_kf, geom.max_mwords,
           geom.chain_lds, geom.min_nc, geom.max_nc, geom.max_cu, geom.max_chain_rows, geom.max_split, geom.step_grid.size(), geom.pan_grid.size(), geom.tile_updates,
           (int)geom.any_lin_fallback);
}

int main(int argc, char** argv) {
    LaunchGeom geom;
    std::vector<vba_problem*> probs;
    std::vector<std::pair<std::string, int>> pending;
    int rc = 0;
    for (int a = 1; a <= argc && !rc; a++) {
        if (a == argc || !strcmp(argv[a], "--")) {   // the batch is complete
            if (!probs.empty()) describe_batch(probs, geom);
            for (vba_problem* P : probs) vba_problem_free(P);
            probs.clear();
        } else if (argv[a][0] == '@') {
            const char* eq = strchr(argv[a], '=');
            if (!eq) { printf("error bad override %s\n", argv[a]); rc = 2; break; }
            pending.emplace_back(std::string(argv[a] + 1, (size_t)(eq - argv[a] - 1)), atoi(eq + 1));
        } else {
            vba_problem* P = nullptr;
            if (vba_problem_load(argv[a], &P)) { printf("error load %s\n", argv[a]); rc = 2; break; }
            probs.push_back(P);
            for (auto& kv : pending)
                if (!override_field(P, kv.first, kv.second)) { printf("error unknown field %s\n", kv.first.c_str()); rc = 2; }
            pending.clear();
        }
    }
    for (vba_problem* P : probs) vba_problem_free(P);
    return rc;
}
