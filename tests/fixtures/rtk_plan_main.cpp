// Prints the plan of a sweep of the two run-time-K paths (hammlet_amd/csrc/hml_rtk_plan.h) for rows of inputs on stdin
// (tests/test_rtk_plan_cpu.py):
//   mode(compat|wide) K D T mix probes hint [knob=value ...]
// -> form C W by_state exp KC pad mix | max_chunks min_L room
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>

#include "hml_rtk_plan.h"

int main() {
    static const char* const form[] = {"sequential", "chunked", "lanes"};
    static const char* const expf_[] = {"glibc", "dev"};
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string mode;
        unsigned long long T, hint;
        int K, D, mix, probes;
        if (!(in >> mode >> K >> D >> T >> mix >> probes >> hint)) continue;
        if (mode != "compat" && mode != "wide") { fprintf(stderr, "unknown mode %s\n", mode.c_str()); return 2; }
        hml_rtk_knobs k;
        std::string kv;
        while (in >> kv) {
            const size_t eq = kv.find('=');
            if (eq == std::string::npos) { fprintf(stderr, "not name=value: %s\n", kv.c_str()); return 2; }
            const std::string name = kv.substr(0, eq);
            const long v = atol(kv.c_str() + eq + 1);
            if (name == "compat_chunks") k.compat_chunks = (int)v;
            else if (name == "compat_warmup") k.compat_warmup = (int)v;
            else if (name == "wide_lanes") k.wide_lanes = (int)v;
            else if (name == "wide_w0") k.wide_w0 = (int)v;
            else if (name == "wide_max_chunks") k.wide_max_chunks = (uint32_t)v;
            else if (name == "wide_lshift") k.wide_lshift = (int)v;
            else { fprintf(stderr, "unknown knob %s\n", name.c_str()); return 2; }
        }
        const hml_rtk_plan p = hml_plan_rtk(k, mode == "wide" ? HML_RTK_WIDE : HML_RTK_COMPAT, K, D, T, mix != 0, probes != 0, (uint32_t)hint);
        char W[32];
        if (p.W == HML_CHUNK_W_ADAPTIVE) snprintf(W, sizeof W, "adaptive"); else snprintf(W, sizeof W, "%u", p.W);
        printf("%s %u %s %d %s %d %d %d | %u %u %llu\n", form[p.form], p.C, W, p.by_state ? 1 : 0, expf_[p.exp], p.KC, p.pad ? 1 : 0, p.mix ? 1 : 0,
               p.wl.max_chunks, p.wl.min_L, (unsigned long long)p.room);
    }
    return 0;
}
