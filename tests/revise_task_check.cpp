// revise_task_check.cpp — which revisions mtr_test_revise takes (mtr_amd/csrc/revise_task.h), as a program of its own (the form a sanitizer build runs).
// Named cases: a task the batch path makes, then that task with ONE field moved just past each bound and just onto it - the refusal must be the
// bound's own, the neighbour on the bound must pass.  Random tasks: the header against a model written here from the reference's conditions
// (find_tandem_repeat_sub's `5 <= coverage && coverage <= 20 && 5 < period`, MAX_PERIOD, the window, the ratio's denominator, the search's k, the
// DP's size) that answers only yes or no; every refusal must come with words, every acceptance without.
#include "../mtr_amd/csrc/revise_task.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

static uint32_t g_rng = 2463534242u;
static uint32_t rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 17; g_rng ^= g_rng << 5; return g_rng >> 4; }      // xorshift32
static int rnd_in(int lo, int hi) { return lo + (int)(rnd() % (uint32_t)(hi - lo + 1)); }

static long g_checks = 0;
static void expect(const char *name, const std::string &got, const char *want)
{
    g_checks++;
    if (got != want) { fprintf(stderr, "FAIL: %s\n  header: \"%s\"\n  wanted: \"%s\"\n", name, got.c_str(), want); exit(1); }
}

struct Task { int32_t rd; int32_t rr[13]; int64_t unit_len; };
static const long long WRAP = 200000000;

static bool model_ok(const Task &t, const std::vector<int32_t> &lens, long long wrap)
{
    if (t.rd < 0 || (size_t)t.rd >= lens.size()) return false;
    const long long L = lens[(size_t)t.rd], rs = t.rr[0], re = t.rr[1], len = t.rr[2], U = t.rr[3], k = t.rr[9];
    if (!(5 < U && U < 500) || t.unit_len != U) return false;
    if (!(0 <= rs && rs <= re && re <= L)) return false;
    for (int f = 5; f <= 8; f++) if (t.rr[f] < 0) return false;
    if ((long long)t.rr[5] + t.rr[6] + t.rr[7] + t.rr[8] <= 0 || len <= 0) return false;
    const long long cov = len / U;
    if (!(5 <= cov && cov <= 20)) return false;
    if (k < 2 || k > 15) return false;
    const long long U2 = 2 * U, rows = re - rs + 1;
    return (U2 + 1) * rows + U2 < wrap;
}

int main(int argc, char **argv)
{
    const int n_random = argc > 1 ? atoi(argv[1]) : 2000;
    const std::vector<int32_t> lens = { 300, 1000, 40 };
    // U = 10, 12 copies: rows 100..219 of read 1
    const Task good = { 1, { 100, 219, 120, 10, 12, 110, 6, 4, 2, 5, 1, 1, 3 }, 10 };
    auto run = [&](const Task &t, long long wrap = WRAP) { return rvt_refusal(t.rd, (int32_t)lens.size(), lens.data(), t.rr, t.unit_len, wrap); };
    auto with = [&](int field, int32_t v) { Task t = good; t.rr[field] = v; return t; };
    auto with_unit = [&](int32_t U, int32_t len) { Task t = good; t.rr[3] = U; t.unit_len = U; t.rr[2] = len; return t; };
    int named = 0;
#define CASE(name, task, want) do { expect(name, run(task), want); named++; } while (0)
    CASE("a task of the batch path", good, "");
    { Task t = good; t.rd = 3; CASE("read behind the batch", t, "read outside the batch"); t.rd = -1; CASE("read -1", t, "read outside the batch"); }
    CASE("period 5", with_unit(5, 60), "period outside 6..499");
    CASE("period 6", with_unit(6, 60), "");
    CASE("period 499", with_unit(499, 499 * 5), "");
    CASE("period 500", with_unit(500, 2500), "period outside 6..499");
    { Task t = good; t.unit_len = 11; CASE("unit of another length", t, "the unit's length is not the period"); }
    CASE("rep_start -1", with(0, -1), "window outside 0 <= rep_start <= rep_end <= L");
    CASE("rep_start 0", with(0, 0), "");
    CASE("rep_end = L", with(1, 1000), "");
    CASE("rep_end = L + 1", with(1, 1001), "window outside 0 <= rep_start <= rep_end <= L");
    CASE("rep_end < rep_start", with(1, 99), "window outside 0 <= rep_start <= rep_end <= L");
    CASE("rep_end = rep_start", with(1, 100), "");
    { Task t = good; t.rr[5] = t.rr[6] = t.rr[7] = t.rr[8] = 0; CASE("no counts", t, "non-positive counts"); t.rr[7] = 1; CASE("one insertion", t, ""); }
    CASE("mis -1", with(6, -1), "non-positive counts");
    CASE("repeat_len 0", with(2, 0), "non-positive counts");
    CASE("coverage 4", with(2, 49), "coverage outside 5..20");
    CASE("coverage 5", with(2, 50), "");
    CASE("coverage 20", with(2, 209), "");
    CASE("coverage 21", with(2, 210), "coverage outside 5..20");
    CASE("k 1", with(9, 1), "k outside 2..15");
    CASE("k 2", with(9, 2), "");
    CASE("k 15", with(9, 15), "");
    CASE("k 16", with(9, 16), "k outside 2..15");
    // (2 * 10 + 1) * 120 + 20 = 2540
    expect("size on the bound", run(good, 2540), "period x rows beyond WrapDPsize"); named++;
    expect("size under the bound", run(good, 2541), ""); named++;

    long refused = 0;
    for (int i = 0; i < n_random; i++) {
        Task t = good;
        t.rd = rnd_in(0, 2);
        const int L = lens[(size_t)t.rd];
        const int U = rnd_in(0, 3) ? rnd_in(6, 60) : rnd_in(1, 520);
        t.rr[3] = U; t.unit_len = rnd_in(0, 15) ? U : U + rnd_in(-1, 1);
        t.rr[0] = rnd_in(-1, L); t.rr[1] = t.rr[0] + rnd_in(-1, L - t.rr[0] + 1);
        t.rr[2] = rnd_in(0, 3) ? U * rnd_in(4, 21) + rnd_in(0, U - 1) : rnd_in(-1, 2);
        for (int f = 5; f <= 8; f++) t.rr[f] = rnd_in(0, 7) ? rnd_in(0, 40) : rnd_in(-1, 0);
        t.rr[9] = rnd_in(0, 7) ? rnd_in(2, 15) : rnd_in(0, 17);
        const long long wrap = rnd_in(0, 7) ? WRAP : rnd_in(1, 60000);
        const std::string why = run(t, wrap);
        g_checks++;
        if (why.empty() != model_ok(t, lens, wrap)) {
            fprintf(stderr, "FAIL: random task %d: header \"%s\", model %s\n  rd %d rr %d %d %d %d . %d %d %d %d k %d unit_len %lld wrap %lld\n", i, why.c_str(),
                    model_ok(t, lens, wrap) ? "accepts" : "refuses", t.rd, t.rr[0], t.rr[1], t.rr[2], t.rr[3], t.rr[5], t.rr[6], t.rr[7], t.rr[8], t.rr[9], (long long)t.unit_len, wrap);
            return 1;
        }
        if (!why.empty()) refused++;
    }
    if (n_random >= 1000 && (refused < n_random / 10 || refused > n_random - n_random / 10)) { fprintf(stderr, "FAIL: %ld of %d random tasks refused: the generator is one-sided\n", refused, n_random); return 1; }
    printf("ok: %d named cases, %d random tasks (%ld refused), %ld checks\n", named, n_random, refused, g_checks);
    return 0;
}
