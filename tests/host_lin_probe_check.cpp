// Sanitizer harness of vba_host::plan_lin_probe (mc_slam_amd/csrc/vba_host_plan.h): plain C++, built by tests/test_host_lin_probe.py
// with g++ -fsanitize=address,undefined.  host_lin_probe_check <file>: one case per line of the file, tokens key=value
//   n= variant= algo= hook=      (hook: PathOverrides::lin_probe, what vba_debug_set_path(h, "lin_probe", v) stores; default -1)
// and one line of output per case: "<plan_lin_probe> <RunPlan::lin_probe of plan_run> <PLAN_INTS>" -- the run plan of an empty
// environment must carry the function's value, and the integers of vba_debug_plan stay the 23 they were.
#include "../mc_slam_amd/csrc/vba_host_plan.h"

#include <cstdio>
#include <fstream>
#include <map>
#include <sstream>
#include <string>

using namespace vba_host;

static const char* no_env(const char*) { return nullptr; }

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    std::ifstream in(argv[1]);
    std::string line;
    Knobs K;
    read_knobs(K, READ_ONCE, no_env);
    read_knobs(K, READ_EACH, no_env);
    while (std::getline(in, line)) {
        std::istringstream ss(line);
        std::string tok;
        std::map<std::string, int> par = {{"n", 1}, {"variant", VBA_VARIANT_PRV_IDP}, {"algo", VBA_ALGO_GN}, {"hook", -1}};
        while (ss >> tok) {
            const size_t eq = tok.find('=');
            if (eq == std::string::npos || !par.count(tok.substr(0, eq))) { printf("error token %s\n", tok.c_str()); return 1; }
            par[tok.substr(0, eq)] = atoi(tok.substr(eq + 1).c_str());
        }
        Overrides ov;
        if (ov.path.lin_probe != -1) { printf("error default %d\n", ov.path.lin_probe); return 1; }
        ov.path.lin_probe = par["hook"];
        const int n = par["n"];
        const UploadPlan u = plan_upload(n, false, ov, K);
        const RunPlan r = plan_run(u, n, par["variant"], par["algo"], ov, K, false, false, 14);
        printf("%d %d %d\n", plan_lin_probe(n, par["variant"], par["algo"], ov.path), r.lin_probe, PLAN_INTS);
    }
    return 0;
}
