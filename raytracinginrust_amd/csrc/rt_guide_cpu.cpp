// csrc/rt_guide_cpu.cpp — the averaged denoising guide on the host: rt_guide.h's specification as code, plain C++ (no HIP include; it is
// also compiled stand-alone under sanitizers by tests/test_guide_host.py).
#include <string>
#include "../../include/rt_amd.h"
#include "rt_guide.h"

namespace rt {

int set_error(const std::string& m);          // rt_host.cpp: rt_last_error()'s message; returns -1

void guide_from_hits_host(const double* hits, uint32_t n_samples, uint64_t n_px, double* guide_out) {
    for (uint64_t p = 0; p < n_px; p++) {
        uint32_t h = 0, hf = 0;
        double st = 0.0, sp[3] = {0.0, 0.0, 0.0}, sn[3] = {0.0, 0.0, 0.0};
        double m = -1.0, o = -1.0;
        bool m_same = true, o_same = true;
        for (uint32_t s = 0; s < n_samples; s++) {                  // ascending: the order is part of the definition
            const double* r = hits + ((uint64_t)s * n_px + p) * GUIDE_DOUBLES;
            if (!(r[0] != 0.0)) continue;
            if (h == 0u) { m = r[11]; o = r[12]; }
            else {
                if (r[11] != m) m_same = false;
                if (r[12] != o) o_same = false;
            }
            h++;
            if (r[8] != 0.0) hf++;
            st += r[1];
            for (int k = 0; k < 3; k++) { sp[k] += r[2 + k]; sn[k] += r[5 + k]; }
        }
        double* g = guide_out + p * GUIDE_DOUBLES;
        const double dh = (double)h;
        g[0] = (h >= 1u && 2ull * h >= n_samples) ? 1.0 : 0.0;
        g[1] = h ? st / dh : 0.0;
        for (int k = 0; k < 3; k++) { g[2 + k] = h ? sp[k] / dh : 0.0; g[5 + k] = h ? sn[k] / dh : 0.0; }
        g[8] = h ? (double)hf / dh : 0.0;
        g[9] = 0.0; g[10] = 0.0;
        g[11] = (h && m_same) ? m : -1.0;
        g[12] = (h && o_same) ? o : -1.0;
        g[13] = -1.0; g[14] = -1.0;
        g[15] = dh;
    }
}

} // namespace rt

extern "C" int rt_guide_from_hits_host(const double* hits, uint32_t n_samples, uint64_t n_px, double* guide_out) {
    if (!hits || !guide_out) return rt::set_error("null argument");
    if (n_samples == 0u) return rt::set_error("n_samples must be >= 1");
    rt::guide_from_hits_host(hits, n_samples, n_px, guide_out);
    return 0;
}
