// Sanitizer harness of the batch policy (mc_slam_amd/csrc/vba_host_plan.h): plain C++, built by tests/test_host_plan.py with
// g++ -fsanitize=address,undefined.  host_plan_check <file>: one command per line of the file, one line of output per command.
// Tokens are key=value: an upper-case key is a variable of the FAKE environment of that line (NAME= sets it to the empty string),
// ov.<field> a hook override, anything else a parameter of the command.
//   plan n= variant= algo= pcg= profile= lane= avail=   -> the PLAN_INTS integers of plan_upload + plan_run (order: plan_ints)
//   groups n= g=                                         -> the ngroups + 1 bounds of group_bounds
//   chunks n=                                            -> the chunk sizes of chunk_bounds under the line's knobs and overrides, then "lanes L"
//   knobs                                                -> "NAME=value" of every knob in table order ((null) for an unset text knob)
//   table                                                -> "NAME:kind:read" of every entry of the table, in its order
//   reads                                                -> process_knobs() once, current_knobs() three times: "NAME=reads" per entry
#include "../mc_slam_amd/csrc/vba_host_plan.h"

#include <cstdio>
#include <cstring>
#include <fstream>
#include <map>
#include <sstream>
#include <string>

using namespace vba_host;

static std::map<std::string, std::string> g_env;
static std::map<std::string, int> g_reads;
static const char* fake_env(const char* name) {
    g_reads[name]++;
    auto it = g_env.find(name);
    return it == g_env.end() ? nullptr : it->second.c_str();
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    std::ifstream in(argv[1]);
    std::string line;
    while (std::getline(in, line)) {
        std::istringstream ss(line);
        std::string cmd, tok;
        ss >> cmd;
        g_env.clear();
        g_reads.clear();
        std::map<std::string, int> par;
        Overrides ov;
        const std::map<std::string, int*> ovf = {{"ov.ll_min", &ov.path.ll_min}, {"ov.no_chain", &ov.path.no_chain}, {"ov.stop_after", &ov.path.stop_after},
            {"ov.chol_step", &ov.path.chol_step}, {"ov.schur_split", &ov.path.schur_split}, {"ov.trsv_old", &ov.path.trsv_old},
            {"ov.pcg_jacobi", &ov.path.pcg_jacobi}, {"ov.streams", &ov.streams}, {"ov.chunk", &ov.chunk}, {"ov.lanes", &ov.lanes}};
        while (ss >> tok) {
            const size_t eq = tok.find('=');
            if (eq == std::string::npos) { printf("error token %s\n", tok.c_str()); return 1; }
            const std::string key = tok.substr(0, eq), val = tok.substr(eq + 1);
            if (key[0] >= 'A' && key[0] <= 'Z') g_env[key] = val;
            else if (ovf.count(key)) *ovf.at(key) = atoi(val.c_str());
            else par[key] = atoi(val.c_str());
        }
        Knobs K;   // the knobs of this line: both read times from the line's environment
        read_knobs(K, READ_ONCE, fake_env);
        read_knobs(K, READ_EACH, fake_env);
        auto P = [&](const char* k, int def) { return par.count(k) ? par[k] : def; };
        if (cmd == "plan") {
            const int n = P("n", 1);
            const UploadPlan u = plan_upload(n, P("pcg", 0) != 0, ov, K);
            const RunPlan r = plan_run(u, n, P("variant", VBA_VARIANT_PRV_IDP), P("algo", VBA_ALGO_GN), ov, K, P("profile", 0) != 0, P("lane", 0) != 0, P("avail", 14));
            long long v[PLAN_INTS];
            plan_ints(u, r, v);
            for (int i = 0; i < PLAN_INTS; i++) printf("%lld%c", v[i], i + 1 < PLAN_INTS ? ' ' : '\n');
        } else if (cmd == "groups") {
            const std::vector<int> b = group_bounds(P("n", 1), P("g", 1));
            for (size_t i = 0; i < b.size(); i++) printf("%d%c", b[i], i + 1 < b.size() ? ' ' : '\n');
        } else if (cmd == "chunks") {
            const std::vector<int> c = chunk_bounds(P("n", 1), chunk_max_of(ov, K), !K.no_ramp, K.chunks);
            for (size_t i = 0; i + 1 < c.size(); i++) printf("%d ", c[i + 1] - c[i]);
            printf("lanes %d\n", lanes_of(ov, K, (int)c.size() - 1));
        } else if (cmd == "knobs") {
#define SHOW(field, name, kind, def, read) show(name, K.field);
            struct { void operator()(const char* n, int v) { printf("%s=%d ", n, v); } void operator()(const char* n, const char* v) { printf("%s=%s ", n, v ? v : "(null)"); } } show;
            VBA_KNOBS(SHOW)
#undef SHOW
            printf("\n");
        } else if (cmd == "table") {
            for (const KnobEntry& e : knob_table)
                printf("%s:%s:%s ", e.name, e.kind == KNOB_FLAG ? "flag" : e.kind == KNOB_INT ? "int" : "text", e.read == READ_ONCE ? "once" : "each");
            printf("\n");
        } else if (cmd == "reads") {
            g_reads.clear();
            (void)process_knobs(fake_env);
            for (int i = 0; i < 3; i++) (void)current_knobs(fake_env);
            for (const KnobEntry& e : knob_table) printf("%s=%d ", e.name, g_reads[e.name]);
            printf("\n");
        } else { printf("error command %s\n", cmd.c_str()); return 1; }
    }
    return 0;
}
