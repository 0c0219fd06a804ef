// unit_motif_check.cpp — the per-unit function of the motif catalogue (mtr_amd/csrc/unit_motif.h) for the host: built by the plain host C++
// compiler into a small shared library and called from tests/test_unit_motif_host.py, which compares it with a brute force over all 2p
// rotations.  With -DUNIT_MOTIF_MAIN it is a program of its own that makes the same comparison in C++ (every string up to length 6 and
// units of 499 and 500 bases): the form a sanitizer build runs.
#include "../mtr_amd/csrc/unit_motif.h"

// n units: unit k = units[unit_off[k] .. unit_off[k + 1]).  Per unit its three values, its hash and where the grouping starts to probe in a
// table of `slots` slots (a power of two); its motif is written at motifs + unit_off[k].
extern "C" void um_check_units(const uint8_t *units, const int64_t *unit_off, int32_t n, int32_t *strand, int32_t *rotation, int32_t *motif_len,
                               uint8_t *motifs, uint64_t *hash, uint32_t slots, uint32_t *start_slot)
{
    for (int32_t k = 0; k < n; k++) {
        uint64_t h = 0;
        const UnitMotif m = unit_motif(units + unit_off[k], (int)(unit_off[k + 1] - unit_off[k]), motifs + unit_off[k], &h);
        strand[k] = m.strand; rotation[k] = m.rotation; motif_len[k] = m.motif_len; hash[k] = h;
        start_slot[k] = um_start_slot(h, slots - 1u);
    }
}

#ifdef UNIT_MOTIF_MAIN
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

static std::string rot(const std::string &s, size_t r) { return s.substr(r) + s.substr(0, r); }
static std::string rc(const std::string &s)
{
    std::string o(s.rbegin(), s.rend());
    for (char &c : o) c = c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : 'A';
    return o;
}
// the definition, word for word: the minimum over all 2p rotations, the forward strand and the smaller rotation first
static void brute(const std::string &u, int &strand, int &rotation, std::string &motif)
{
    strand = 0; rotation = 0; motif.clear();
    const size_t p = u.size();
    if (p == 0) return;
    const std::string s[2] = { u, rc(u) };
    std::string best = u;
    for (int st = 0; st < 2; st++)
        for (size_t r = 0; r < p; r++) {
            const std::string c = rot(s[st], r);
            if (c < best) { best = c; strand = st; rotation = (int)r; }
        }
    size_t d = 1;
    while (p % d || rot(best, d) != best) d++;
    motif = best.substr(0, d);
}
static long g_checked = 0;
static bool check(const std::string &u)
{
    int st, r; std::string want;
    brute(u, st, r, want);
    std::vector<uint8_t> got(u.size() + 1, 0xee);
    uint64_t h = 0, h2 = 0;
    const UnitMotif m = unit_motif((const uint8_t *)u.data(), (int)u.size(), got.data(), &h);
    (void)unit_motif((const uint8_t *)want.data(), (int)want.size(), nullptr, &h2);       // a motif is its own motif: the same hash
    g_checked++;
    const bool ok = m.strand == st && m.rotation == r && m.motif_len == (int)want.size() && memcmp(got.data(), want.data(), want.size()) == 0 &&
                    got[want.size()] == 0xee && h == h2 && m.rotation < (m.motif_len ? m.motif_len : 1);
    if (!ok) fprintf(stderr, "unit %s: got (%d, %d, %d), want (%d, %d, %s)\n", u.c_str(), m.strand, m.rotation, m.motif_len, st, r, want.c_str());
    return ok;
}
int main()
{
    bool ok = check("");
    for (int p = 1; p <= 6; p++)
        for (int v = 0; v < (1 << (2 * p)); v++) {
            std::string u((size_t)p, 'A');
            for (int t = 0; t < p; t++) u[(size_t)t] = "ACGT"[(v >> (2 * t)) & 3];
            ok = check(u) && ok;
        }
    uint32_t x = 12345u;
    auto rnd = [&]() { x = x * 1664525u + 1013904223u; return (x >> 24) & 3u; };
    for (int p : { 499, 500 })
        for (int root : { 1, 2, 4, 5, 100, 250, 499, 500 }) {
            if (p % root) continue;
            std::string r((size_t)root, 'A'), u;
            for (char &c : r) c = "ACGT"[rnd()];
            while ((int)u.size() < p) u += r;
            ok = check(u) && ok;
        }
    ok = check(std::string(499, 'T') + "A") && ok;
    ok = check(std::string(500, 'A')) && ok;
    ok = check(std::string(500, 'T')) && ok;
    printf("%ld units checked: %s\n", g_checked, ok ? "ok" : "FAILED");
    return ok ? 0 : 1;
}
#endif
