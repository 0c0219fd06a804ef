// file_state_check.cpp — the file state of file-order mode (mtr_amd/csrc/file_state.h) against a brute-force model of the reference's two
// whole-file buffers, on the CPU.  Built and run by tests/test_file_state_host.py with the address and undefined-behaviour sanitizers.
//
// The model is two flat arrays with a high-water mark each: inputString_w_rand (W) and orgInputString (O).  A read of length L first
// reads W[E .. reach) below W's mark and O[L], O[L + 1] (a position nobody wrote is 0), then writes left_at(itself, p) for p < E into W and
// its codes into O[0 .. L).  Asserted for every file, under several ways of cutting it into batches:
//   (a) the host feed's tail, tail_off and after-bases of every read equal the model's;
//   (b) the device feed's segments, expanded through left_at with their owners' codes, equal the same entries, and its after-owners
//       hold the model's bases at L and L + 1;
//   (c) the staircase after the file is the same whatever the cuts (one batch, random cuts, every read alone) and whichever feed;
//   (d) planning a batch without adopting it leaves the state as it was.
// usage: file_state_check <random files> <of them with a 720000-base read>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <utility>
#include <vector>

#include "../mtr_amd/csrc/file_state.h"

#define CHECK(cond, ...) do { if (!(cond)) { fprintf(stderr, "FAILED %s:%d: %s\n  ", __FILE__, __LINE__, #cond); fprintf(stderr, __VA_ARGS__); \
    fputc('\n', stderr); exit(1); } } while (0)

typedef std::vector<std::pair<int, int>> Cuts;
struct Read { std::vector<uint8_t> codes; std::vector<uint16_t> tail; uint8_t after[2]; };      // tail, after: what the model says it finds
struct TSeg { const uint8_t *words; int64_t t0; int32_t p0, L, r, N; };                         // FoSeg / FoAfter with codes for words
struct TAfter { const uint8_t *w[2]; };

static uint64_t g_rng = 0x9e3779b97f4a7c15ull;
static uint32_t rnd(uint32_t n) { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17; return (uint32_t)((g_rng >> 11) % n); }

static mtr_file_state g_fs;            // the one state, emptied for every feed (its copy of the MT19937 stream stays)
static mtr_file_state &fresh_state() { g_fs.stairs.clear(); g_fs.reads_seen = 0; g_fs.kind = mtr_file_state::UNFED; return g_fs; }

// ---- the model ----
static void model(std::vector<Read> &file)
{
    static std::vector<uint16_t> W((size_t)MTRC_MAX_INPUT_LENGTH + 64);
    static std::vector<uint8_t> O((size_t)MTRC_MAX_SUPPORTED_LENGTH + 2);
    const mtr_file_state &fs = g_fs;
    int64_t w_top = 0, o_top = 0;
    for (Read &rd : file) {
        const int32_t L = (int32_t)rd.codes.size();
        const int64_t r = L < 1000 ? 100 : L / 10, n = L + 2 * r, N = std::min<int64_t>(L + 4 * r, 1000000), E = std::max(N, n);
        int wtop = 0;
        for (int w = 5; w <= 10240 && w < L / 2; w *= 2) wtop = w;
        const int64_t reach = std::max<int64_t>(L + r + 2 * wtop + 8, E);
        rd.tail.clear();
        for (int64_t p = E; p < reach && p < w_top; p++) rd.tail.push_back(W[(size_t)p]);
        for (int d = 0; d < 2; d++) rd.after[d] = L + d < o_top ? O[(size_t)(L + d)] : 0;
        const FileStair me(L);
        CHECK(me.r == r && me.n == n && me.N == N && me.E == E, "geometry of L = %d", L);
        for (int64_t p = 0; p < E; p++) W[(size_t)p] = (uint16_t)fs.left_at(me, rd.codes.data(), p);
        std::copy(rd.codes.begin(), rd.codes.end(), O.begin());
        w_top = std::max(w_top, E); o_top = std::max<int64_t>(o_top, L);
    }
}

// ---- the two feeds, batch by batch ----
struct Batch { std::vector<uint8_t> bases; std::vector<int64_t> offsets; std::vector<int32_t> lens; std::vector<uint16_t> tail; std::vector<int64_t> tail_off;
               std::vector<uint8_t> after; };
static Batch batch_of(const std::vector<Read> &file, int lo, int hi)
{
    Batch b;
    b.tail_off.push_back(0);
    for (int i = lo; i < hi; i++) {
        b.offsets.push_back((int64_t)b.bases.size()); b.lens.push_back((int32_t)file[i].codes.size());
        b.bases.insert(b.bases.end(), file[i].codes.begin(), file[i].codes.end());
        b.tail.insert(b.tail.end(), file[i].tail.begin(), file[i].tail.end());
        b.tail_off.push_back((int64_t)b.tail.size());
        b.after.push_back(file[i].after[0]); b.after.push_back(file[i].after[1]);
    }
    return b;
}

struct Snapshot { std::vector<FileStair> stairs; int64_t reads_seen; int kind; };
static Snapshot snapshot(const mtr_file_state &fs) { return Snapshot{ fs.stairs, fs.reads_seen, fs.kind }; }
static void check_unchanged(const mtr_file_state &fs, const Snapshot &s, const char *what)
{
    CHECK(fs.reads_seen == s.reads_seen && fs.kind == s.kind && fs.stairs.size() == s.stairs.size(), "%s: planning changed the state", what);
    for (size_t k = 0; k < s.stairs.size(); k++) {
        const FileStair &a = fs.stairs[k], &b = s.stairs[k];
        CHECK(a.L == b.L && a.r == b.r && a.N == b.N && a.n == b.n && a.E == b.E && a.codes == b.codes && a.woff == b.woff && a.read == b.read,
              "%s: planning changed stair %zu", what, k);
    }
}

static std::vector<FileStair> feed_host(const std::vector<Read> &file, const Cuts &cuts, const char *what)
{
    mtr_file_state &fs = fresh_state();
    for (const auto &c : cuts) {
        const Batch b = batch_of(file, c.first, c.second);
        const int32_t n = (int32_t)b.lens.size();
        const Snapshot before = snapshot(fs);
        mtr_file_state::HostPlan p;
        fs.plan_host(b.bases.data(), b.offsets.data(), b.lens.data(), n, p);
        check_unchanged(fs, before, what);                                                      // (d)
        CHECK(p.tail_off == b.tail_off, "%s, host feed, reads %d..%d: tail_off", what, c.first, c.second);      // (a)
        CHECK(p.tail == b.tail, "%s, host feed, reads %d..%d: tail", what, c.first, c.second);
        CHECK(p.after == b.after, "%s, host feed, reads %d..%d: after-bases", what, c.first, c.second);
        fs.adopt_host(std::move(p.work), b.bases.data(), b.offsets.data(), n);
        CHECK(fs.kind == mtr_file_state::HOST_FED && fs.reads_seen == c.second, "%s: host state after reads ..%d", what, c.second);
    }
    return fs.stairs;
}

static std::vector<FileStair> feed_device(const std::vector<Read> &file, const Cuts &cuts, const char *what)
{
    mtr_file_state &fs = fresh_state();
    for (const auto &c : cuts) {
        const Batch b = batch_of(file, c.first, c.second);
        const int32_t n = (int32_t)b.lens.size();
        const Snapshot before = snapshot(fs);
        std::vector<FileStair> work; std::vector<TSeg> segs; std::vector<int64_t> tail_off; std::vector<TAfter> own;
        // (here a stair of the state keeps its codes where the library keeps its words in device memory)
        fs.plan_device(b.lens.data(), n, [&](const FileStair &o) { return o.read >= 0 ? b.bases.data() + b.offsets[(size_t)o.read] : o.codes->data(); },
                       work, segs, tail_off, own);
        check_unchanged(fs, before, what);                                                      // (d)
        CHECK(tail_off == b.tail_off, "%s, device feed, reads %d..%d: tail_off", what, c.first, c.second);      // (b)
        for (size_t j = 0; j < segs.size(); j++) {
            const TSeg &s = segs[j];
            const int64_t end = j + 1 < segs.size() ? segs[j + 1].t0 : (int64_t)b.tail.size();
            const FileStair owner(s.L);
            CHECK(owner.r == s.r && owner.N == s.N && s.t0 < end && (j == 0 ? s.t0 == 0 : segs[j - 1].t0 < s.t0), "%s, device feed: segment %zu", what, j);
            for (int64_t t = s.t0; t < end; t++)
                CHECK(fs.left_at(owner, s.words, s.p0 + (t - s.t0)) == b.tail[(size_t)t], "%s, device feed, reads %d..%d: tail entry %lld (segment %zu)", what,
                      c.first, c.second, (long long)t, j);
        }
        CHECK(segs.empty() == b.tail.empty(), "%s, device feed: segments and entries", what);
        for (int32_t i = 0; i < n; i++)
            for (int d = 0; d < 2; d++) {
                const uint8_t *w = own[(size_t)i].w[d];
                CHECK((w ? w[b.lens[(size_t)i] + d] : 0) == b.after[(size_t)i * 2 + (size_t)d], "%s, device feed, read %d: base after + %d", what, c.first + i, d);
            }
        // what the library's commit does: the survivors stay, the new stairs are stacked behind them
        const mtr_file_state::Survivors s = mtr_file_state::survivors(work);
        CHECK(s.kept <= fs.stairs.size() && s.top == (s.kept ? fs.stairs[s.kept - 1].woff + mtr_packed_words(fs.stairs[s.kept - 1].L) : 0), "%s: survivors", what);
        int64_t at = s.top;
        for (size_t k = s.kept; k < work.size(); k++) {
            FileStair &o = work[k];
            const uint8_t *codes = b.bases.data() + b.offsets[(size_t)o.read];
            o.codes = std::make_shared<const std::vector<uint8_t>>(codes, codes + o.L);
            o.woff = at; o.read = -1; at += mtr_packed_words(o.L);
        }
        CHECK(at == s.top + s.fresh, "%s: words of the new stairs", what);
        fs.stairs = std::move(work); fs.reads_seen += n; fs.kind = mtr_file_state::DEVICE_FED;
        CHECK(fs.store_top() == at, "%s: top of the store", what);
    }
    return fs.stairs;
}

static void check_same_stairs(const std::vector<FileStair> &a, const std::vector<FileStair> &b, const char *what, const char *which)
{
    CHECK(a.size() == b.size(), "%s: %s leaves %zu stairs, one batch from the host %zu", what, which, b.size(), a.size());
    for (size_t k = 0; k < a.size(); k++)
        CHECK(a[k].L == b[k].L && a[k].r == b[k].r && a[k].N == b[k].N && a[k].n == b[k].n && a[k].E == b[k].E && *a[k].codes == *b[k].codes && b[k].read < 0,
              "%s: %s, stair %zu", what, which, k);
}

static void check_file(const std::vector<int32_t> &lens, const std::vector<Cuts> &splits, const char *what)
{
    std::vector<Read> file(lens.size());
    for (size_t i = 0; i < lens.size(); i++) {
        file[i].codes.resize((size_t)lens[i]);
        for (uint8_t &c : file[i].codes) c = (uint8_t)rnd(4);
    }
    model(file);
    const int n = (int)lens.size();
    Cuts one = { { 0, n } }, each;
    for (int i = 0; i < n; i++) each.push_back({ i, i + 1 });
    const std::vector<FileStair> want = feed_host(file, one, what);
    for (size_t k = 0; k + 1 < want.size(); k++) CHECK(want[k].L > want[k + 1].L && want[k].E > want[k + 1].E, "%s: stairs %zu, %zu do not descend", what, k, k + 1);
    check_same_stairs(want, feed_device(file, one, what), what, "one batch from the device");       // (c)
    check_same_stairs(want, feed_host(file, each, what), what, "every read alone from the host");
    check_same_stairs(want, feed_device(file, each, what), what, "every read alone from the device");
    for (const Cuts &cuts : splits) {
        check_same_stairs(want, feed_host(file, cuts, what), what, "a split from the host");
        check_same_stairs(want, feed_device(file, cuts, what), what, "a split from the device");
    }
    // the skips see lengths only and leave the same stairs
    std::vector<FileStair> skipped = mtr_file_state::skipped({}, lens.data(), n);
    CHECK(skipped.size() == want.size(), "%s: skipped", what);
    for (size_t k = 0; k < want.size(); k++) CHECK(skipped[k].L == want[k].L && skipped[k].read >= 0 && lens[(size_t)skipped[k].read] == want[k].L, "%s: skipped stair %zu", what, k);
}

int main(int argc, char **argv)
{
    const int n_files = argc > 1 ? atoi(argv[1]) : 200, n_long = argc > 2 ? atoi(argv[2]) : 6;
    mt_bases(g_fs.mt, MTR_MT_BASES);
    // TAIL_LENS, WORD_EDGE_LENS and the three splits of tests/test_gpu_file_order_device.py
    const std::vector<int32_t> tail_lens = { 720000, 60000, 12000, 10100, 600, 2000, 600, 910, 600, 820, 600, 1000, 600, 999, 600, 900, 610, 600, 617, 616, 615, 614,
                                             601, 600, 599 };
    const std::vector<int32_t> word_edge_lens = { 2000, 641, 640, 639, 31, 15 };
    check_file(tail_lens, { { { 0, 1 }, { 1, 5 }, { 5, (int)tail_lens.size() } } }, "TAIL_LENS");
    check_file(word_edge_lens, { { { 0, 2 }, { 2, (int)word_edge_lens.size() } } }, "WORD_EDGE_LENS");
    // random files of 1..40 reads, lengths from the classes below, random cuts; a 720000-base read in the first n_long files only (one each)
    long reads = 0;
    for (int f = 0; f < n_files; f++) {
        const int n = 1 + (int)rnd(40);
        std::vector<int32_t> lens((size_t)n);
        for (int32_t &L : lens)
            switch (rnd(8)) {
            case 0: case 1: L = 1 + (int32_t)rnd(50); break;
            case 2: case 3: L = 599 + (int32_t)rnd(43); break;
            case 4: L = 999 + (int32_t)rnd(3); break;
            case 5: case 6: L = 10100; break;
            default: L = 60000; break;
            }
        if (f < n_long) lens[rnd((uint32_t)n)] = 720000;
        Cuts cuts;
        for (int lo = 0; lo < n; ) { const int hi = std::min(n, lo + 1 + (int)rnd(8)); cuts.push_back({ lo, hi }); lo = hi; }
        const std::string what = "random file " + std::to_string(f);
        check_file(lens, { cuts }, what.c_str());
        reads += n;
    }
    printf("ok: 2 fixed files, %d random files (%d with a 720000-base read), %ld reads\n", n_files, std::min(n_files, n_long), reads);
    return 0;
}
