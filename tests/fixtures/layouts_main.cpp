// Prints the layouts of the carved device buffers (hammlet_amd/csrc/hml_layouts.h) for rows of inputs on stdin
// (tests/test_layouts_cpu.py):
//   cchunk mode(compat|wide) K cap wide_lshift wide_max_chunks | clists K cap | wa | wave_total tiles
// -> bytes on a null base, bytes on a real base, then the offset of every view from the real base, in the order the kernels'
//    structures name them here.  Nothing is dereferenced: the real base is a small aligned allocation.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>

#include "hml_layouts.h"

static char* g_base;
static unsigned long long off(const void* p) { return (unsigned long long)((uintptr_t)p - (uintptr_t)g_base); }

int main() {
    g_base = (char*)aligned_alloc(256, 256);
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string what;
        if (!(in >> what)) continue;
        if (what == "cchunk") {
            std::string mode; int K, lshift; unsigned long long cap, maxc;
            if (!(in >> mode >> K >> cap >> lshift >> maxc)) return 2;
            hml_rtk_knobs k; k.wide_lshift = lshift; k.wide_max_chunks = (uint32_t)maxc;
            const int m = mode == "wide" ? HML_RTK_WIDE : HML_RTK_COMPAT;
            const hml_wl_geometry g = hml_plan_wl_geometry(k, K);
            const hml_cchunk_layout a = hml_layout_cchunk(nullptr, m, g, cap, K), b = hml_layout_cchunk(g_base, m, g, cap, K);
            printf("%llu %llu %llu %llu %llu %llu %llu %llu %llu | chunks %llu tot_bytes %llu plane %llu\n", (unsigned long long)a.bytes, (unsigned long long)b.bytes, off(b.ch.entry),
                   off(b.ch.exitv), off(b.ch.nfb), off(b.ch.in_state), off(b.ch.out_state), off(b.ch.bad), off(b.ch.tot), (unsigned long long)hml_cchunk_chunks(m, g, cap),
                   (unsigned long long)b.tot_bytes, (unsigned long long)hml_wl_plane_floats(g, cap, K));
        } else if (what == "clists") {
            int K; unsigned long long cap;
            if (!(in >> K >> cap)) return 2;
            const hml_clists_layout a = hml_layout_clists(nullptr, cap, K), b = hml_layout_clists(g_base, cap, K);
            printf("%llu %llu %llu %llu %llu %llu %llu %llu\n", (unsigned long long)a.bytes, (unsigned long long)b.bytes, off(b.pl.sx), off(b.pl.sq), off(b.pl.n), off(b.pl.offdiag),
                   off(b.pl.tile_count), off(b.pl.state_off));
        } else if (what == "wa") {
            const hml_wa_layout a = hml_layout_wa(nullptr), b = hml_layout_wa(g_base);
            printf("%llu %llu %llu %llu\n", (unsigned long long)a.bytes, (unsigned long long)b.bytes, off(b.A), off(b.gtab));
        } else if (what == "wave_total") {
            unsigned long long tiles;
            if (!(in >> tiles)) return 2;
            const hml_wave_total_layout a = hml_layout_wave_total(nullptr, tiles), b = hml_layout_wave_total(g_base, tiles);
            printf("%llu %llu %llu %llu %llu\n", (unsigned long long)a.bytes, (unsigned long long)b.bytes, off(b.wave_total), off(b.tile_before), off(b.tile_prev));
        } else { fprintf(stderr, "unknown buffer %s\n", what.c_str()); return 2; }
    }
    free(g_base);
    return 0;
}
