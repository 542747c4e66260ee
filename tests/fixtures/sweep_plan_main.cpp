// Prints the plan of a sweep (hammlet_amd/csrc/hml_sweep_plan.h) for rows of inputs on stdin (tests/test_sweep_plan_cpu.py):
//   hint T D mix alone_on_device wait_expired [knob=value ...]
// -> geometry L lshift cstride keep_gsc trellis fused_wanted scan first_pass counts chain_levels mix params_spread | plan's float_stream many_blocks |
//    the predicates' | fields of the plan that operator== fails to tell apart (none: "-")
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>

#include "hml_sweep_plan.h"

// every field of the plan changed on its own must make two plans unequal: the names of those that do not
static std::string fields_equal_ignores(const hml_sweep_plan& p) {
    std::string missed;
#define HML_FLIP(field, value) { hml_sweep_plan q = p; q.field = value; if (q == p) missed += std::string(missed.empty() ? "" : ",") + #field; }
    HML_FLIP(geo, (uint8_t)(p.geo + 1)) HML_FLIP(L, p.L + 1) HML_FLIP(lay.lshift, p.lay.lshift + 1u) HML_FLIP(lay.cstride, p.lay.cstride + 64u)
    HML_FLIP(mix, !p.mix) HML_FLIP(many_blocks, !p.many_blocks) HML_FLIP(float_stream, !p.float_stream) HML_FLIP(keep_gsc, !p.keep_gsc)
    HML_FLIP(trellis, !p.trellis) HML_FLIP(fused_wanted, !p.fused_wanted) HML_FLIP(scan, (uint8_t)(p.scan + 1)) HML_FLIP(first_pass, (uint8_t)(p.first_pass + 1))
    HML_FLIP(counts, (uint8_t)(p.counts + 1)) HML_FLIP(params_spread, !p.params_spread)
#undef HML_FLIP
    return missed.empty() ? "-" : missed;
}

static void set_L(hml_fwd_geo& g, int L) { g.L = L; g.lay.lshift = 0; while ((1 << g.lay.lshift) < L) ++g.lay.lshift; }

int main() {
    static const char* const geo[] = {"sparse", "mid", "dense", "many"};
    static const char* const scan[] = {"summary", "float", "flags"};
    static const char* const pass[] = {"rows<true>", "rows<false>", "tile"};
    static const char* const counts[] = {"multivariate", "dense", "plain"};
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        unsigned long long hint, T;
        int D, mix, alone, expired;
        if (!(in >> hint >> T >> D >> mix >> alone >> expired)) continue;
        hml_sweep_knobs k;
        std::string kv;
        while (in >> kv) {
            const size_t eq = kv.find('=');
            if (eq == std::string::npos) { fprintf(stderr, "not name=value: %s\n", kv.c_str()); return 2; }
            const std::string name = kv.substr(0, eq);
            const long v = atol(kv.c_str() + eq + 1);
            if (name == "L_sparse") set_L(k.geo[HML_GEO_SPARSE], (int)v);
            else if (name == "L_mid") set_L(k.geo[HML_GEO_MID], (int)v);
            else if (name == "L_dense") set_L(k.geo[HML_GEO_DENSE], (int)v);
            else if (name == "mid_min_blocks") k.mid_min_blocks = (uint32_t)v;
            else if (name == "dense_min_blocks") k.dense_min_blocks = (uint32_t)v;
            else if (name == "late_rescale") k.late_rescale = v != 0;
            else if (name == "tre_fused") k.tre_fused = v != 0;
            else if (name == "tre_rows") k.tre_rows = v != 0;
            else if (name == "use_keys") k.use_keys = v != 0;
            else if (name == "summary_always") k.summary_always = v != 0;
            else if (name == "stage_bits") k.stage_bits = v != 0;
            else if (name == "fused_blocks") k.fused_blocks = v != 0;
            else if (name == "fused_keep") k.fused_keep = v != 0;
            else if (name == "params_spread") k.params_spread = v != 0;
            else if (name == "cstride") { for (hml_fwd_geo& g : k.geo) g.lay.cstride = (uint32_t)v; }
            else { fprintf(stderr, "unknown knob %s\n", name.c_str()); return 2; }
        }
        const hml_sweep_plan p = hml_plan_sweep(k, T, D, mix != 0, (uint32_t)hint, alone != 0, expired != 0);
        if (!(p == p)) return 3;
        printf("%s %d %u %u %d %d %d %s %s %s %d %d %d | %d %d | %d %d | %s\n", geo[p.geo], p.L, p.lay.lshift, p.lay.cstride, p.keep_gsc ? 1 : 0, p.trellis ? 1 : 0,
               p.fused_wanted ? 1 : 0, scan[p.scan], pass[p.first_pass], counts[p.counts], p.many_blocks ? 2 : 1, p.mix ? 1 : 0, p.params_spread ? 1 : 0,
               p.float_stream ? 1 : 0, p.many_blocks ? 1 : 0, hml_plan_float_stream(k, T, (uint32_t)hint) ? 1 : 0, hml_plan_many_blocks(k, (uint32_t)hint) ? 1 : 0,
               fields_equal_ignores(p).c_str());
    }
    return 0;
}
