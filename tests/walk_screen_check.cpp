// walk_screen_check.cpp — the per-range function of the dead-range screen (mtr_amd/csrc/walk_screen.h) for the host: built by the plain host C++
// compiler into a small shared library and called from tests/test_walk_screen_host.py, which compares it with the CPU oracle range by range.
#include "../mtr_amd/csrc/walk_screen.h"

// n ranges of ONE read (pk: its bases 2 bits each, first base in the top bits of word 0, at least one zero word behind the last).  Per range:
// applies = the rule covers it; max_freq and dead are written only where it does (else -1).
extern "C" void ws_check_ranges(const uint32_t *pk, int32_t L, int32_t n, const int32_t *qs, const int32_t *qe, const int32_t *w,
                                int32_t *applies, int32_t *max_freq, int32_t *dead)
{
    for (int32_t i = 0; i < n; i++) {
        applies[i] = ws_applies(qs[i], qe[i], w[i]) ? 1 : 0;
        max_freq[i] = -1; dead[i] = -1;
        if (!applies[i]) continue;
        int mf = -1;
        dead[i] = ws_range_dead(pk, L, qs[i], qe[i], w[i], &mf) ? 1 : 0;
        max_freq[i] = mf;
    }
}
// the k range of a window as the kernels take it
extern "C" void ws_k_range(int32_t w, int32_t *min_k, int32_t *max_k) { int a, b; k2_k_range(w, a, b); *min_k = a; *max_k = b; }
