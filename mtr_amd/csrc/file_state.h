// file_state.h — file-order mode: the host shadow of the reference's process-wide buffers.  Plain C++17, nothing of HIP: the state,
// its staircase and the planning of a batch compile and run without a GPU (tests/file_state_check.cpp).
//
// The reference keeps inputString_w_rand and orgInputString for the whole file (handle_one_file.c:85, mTR.h:65-67).  A
// read rewrites [0, E) of the first (E = max(L + 2r, min(L + 4r, 1e6)), fill_directional_index.c:137-169, three times:
// k = 1, 3, 5, so it LEAVES the k = 5 encoding) and [0, L) of the second; the passes of the next read look up to
// L + r + 2w - k (:232) and its DPs up to org[L + 1], i.e. into what the most recent LONGER read left there.
// That state is a staircase: of all earlier reads only those longer than every read after them still show.
//
// A state is fed either from the host (mtr_upload_batch_in_file, mtr_file_state_skip: every stair keeps its base codes here) or from
// device memory (mtr_upload_batch_device_in_file, mtr_upload_fasta_device_in_file, mtr_file_state_skip_device).  A device-fed state
// keeps the stairs' geometry here - lengths only - and their 2-bit words in device memory of its own (d_store): a stack like the
// staircase itself, stair k at words [woff, woff + mtr_packed_words(L)), so the survivors of a batch are a prefix of it and the
// new stairs are appended, device to device, from the batch's packed image.  Its bases never reach the host.
//
// Both feeds plan a batch the same way: walk() and push() over a working copy of the staircase, read by read in file order (plan_host,
// plan_device), and hand the copy to the state (adopt) after the last step of the upload that can fail.  walk() is the only place that
// knows how far a read looks and which stairs it sees there.
#pragma once
#include <algorithm>
#include <cstdint>
#include <memory>
#include <vector>

#include "../../include/mtr_hip.h"
#include "mtr_common.h"

// ---- MT19937 (reference MT.h = stock mt19937ar), host-precomputed base stream -------------------------
static inline void mt_bases(std::vector<uint8_t> &out, size_t n)
{
    uint32_t s[624];
    s[0] = 0u;                                                   // init_genrand(0), fill_directional_index.c:140
    for (int i = 1; i < 624; i++) s[i] = 1812433253u * (s[i - 1] ^ (s[i - 1] >> 30)) + (uint32_t)i;
    int idx = 624;
    out.resize(n);
    for (size_t t = 0; t < n; t++) {
        if (idx >= 624) {
            for (int i = 0; i < 624; i++) {
                uint32_t y = (s[i] & 0x80000000u) | (s[(i + 1) % 624] & 0x7fffffffu);
                s[i] = s[(i + 397) % 624] ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
            }
            idx = 0;
        }
        uint32_t y = s[idx++];
        y ^= y >> 11; y ^= (y << 7) & 0x9d2c5680u; y ^= (y << 15) & 0xefc60000u; y ^= y >> 18;
        out[t] = (uint8_t)(y % 4u);                              // random_base(), fill_directional_index.c:131
    }
}
#define MTR_MT_BASES ((size_t)MTRC_MAX_INPUT_LENGTH + 2 * 100000 + 64)      // as many as any read's buffer takes from the stream

// One stair: the geometry of the read that left it, and what names the owner of its bases - the codes themselves (a stair of a host-fed
// state), its words in d_store (a stair of a device-fed state) or, in the working staircase of a batch, a read of that batch.
struct FileStair {
    int32_t L = 0, r = 0; int64_t N = 0, n = 0, E = 0;
    std::shared_ptr<const std::vector<uint8_t>> codes;
    int64_t woff = 0;
    int32_t read = -1;                       // >= 0: read `read` of the batch being planned, nothing of it stored yet
    explicit FileStair(int32_t len, int32_t of_read = -1)
        : L(len), r(mtrc_rand_len(len)), N(std::min<int64_t>((int64_t)len + 4 * (int64_t)r, MTRC_MAX_INPUT_LENGTH)), n((int64_t)len + 2 * r), E(std::max(N, n)), read(of_read) {}
};

// What the next read of some length finds beyond its own part of the two buffers (walk): the entries [E, reach) of inputString_w_rand
// as segments cut where their owner changes, in entry order, and the owners of positions L and L + 1 of orgInputString (nullptr: nobody
// wrote there, 'A' = 0).  The pointers are into the staircase walked and hold until it changes.
struct FileWalk {
    struct Seg { const FileStair *owner; int64_t p0, count; };
    std::vector<Seg> segs;
    const FileStair *after[2];
};

struct mtr_file_state {
    enum Kind { UNFED = 0, HOST_FED = 1, DEVICE_FED = 2 };
    std::vector<FileStair> stairs;           // E (and L) strictly increasing from back() = most recent to front()
    std::vector<uint8_t> mt;                 // the MT19937 base stream (same as the device's)
    int64_t reads_seen = 0;
    int kind = UNFED, device = -1;           // fixed by the first feed; device: the GPU of the context that fed it
    uint32_t *d_store = nullptr; int64_t store_cap = 0;      // device-fed: the stairs' words, capacity in words
    int64_t store_top() const { return stairs.empty() ? 0 : stairs.back().woff + mtr_packed_words(stairs.back().L); }

    int raw(const FileStair &e, const uint8_t *codes, int64_t q) const
    {   // the buffer before the rolling encode, as k1_raw (k1_ranges.hip.inc)
        if (q < e.r) return mt[(size_t)(e.N + q)];
        if (q < e.r + e.L) return codes[(size_t)(q - e.r)];
        if (q < e.n) return mt[(size_t)(e.N + e.r + (q - e.r - e.L))];
        return mt[(size_t)q];                // q < N
    }
    int left_at(const FileStair &e, const uint8_t *codes, int64_t p) const
    {   // what the read left at p < E: the 5-mer code where one was formed (:162-168), else the raw entry
        if (p < e.n - 4) { int v = 0; for (int t = 0; t < 5; t++) v = 4 * v + raw(e, codes, p + t); return v; }
        return raw(e, codes, p);
    }

    static void walk(const std::vector<FileStair> &work, int32_t L, FileWalk &out)
    {
        const FileStair me(L);
        int wtop = 0;
        for (int w = MTRC_MIN_WINDOW; w <= MTRC_MAX_WINDOW && w < L / 2; w *= 2) wtop = w;
        const int64_t reach = std::max<int64_t>((int64_t)L + me.r + 2 * wtop + 8, me.E);      // = ncode of k1_read
        out.segs.clear();
        int64_t cur = me.E;
        for (size_t k = work.size(); k-- > 0 && cur < reach; ) {
            if (work[k].E <= cur) continue;
            const int64_t end = std::min(work[k].E, reach);
            out.segs.push_back(FileWalk::Seg{ &work[k], cur, end - cur });
            cur = end;
        }
        for (int d = 0; d < 2; d++) {
            out.after[d] = nullptr;
            for (size_t k = work.size(); k-- > 0; )
                if (work[k].L > L + d) { out.after[d] = &work[k]; break; }
        }
    }
    // what a read leaves behind it: every stair that is not longer disappears under it
    static void push(std::vector<FileStair> &work, FileStair s)
    {
        while (!work.empty() && work.back().L <= s.L) work.pop_back();
        work.push_back(std::move(s));
    }
    // the staircase behind reads that nobody plans for (the skips): lengths are all it takes
    static std::vector<FileStair> skipped(std::vector<FileStair> work, const int32_t *lens, int32_t n)
    {
        for (int32_t i = 0; i < n; i++) push(work, FileStair(lens[i], i));
        return work;
    }

    // ---- the host feed: reads as base codes, read i = bases[offsets[i] .. + lens[i]) ----
    struct HostPlan { std::vector<FileStair> work; std::vector<uint16_t> tail; std::vector<int64_t> tail_off; std::vector<uint8_t> after; };
    // per read its tail (entries [tail_off[i], tail_off[i + 1]) of p.tail) and its two after-bases; p.work: the staircase after the batch
    void plan_host(const uint8_t *bases, const int64_t *offsets, const int32_t *lens, int32_t n, HostPlan &p) const
    {
        auto codes = [&](const FileStair &o) { return o.read >= 0 ? bases + offsets[o.read] : o.codes->data(); };
        p.work = stairs; p.tail.clear();
        p.tail_off.assign((size_t)n + 1, 0); p.after.assign((size_t)n * 2, 0);
        FileWalk w;
        for (int32_t i = 0; i < n; i++) {
            walk(p.work, lens[i], w);
            for (const FileWalk::Seg &s : w.segs) {
                const uint8_t *c = codes(*s.owner);
                for (int64_t q = s.p0; q < s.p0 + s.count; q++) p.tail.push_back((uint16_t)left_at(*s.owner, c, q));
            }
            p.tail_off[(size_t)i + 1] = (int64_t)p.tail.size();
            for (int d = 0; d < 2; d++)
                if (w.after[d]) p.after[(size_t)i * 2 + (size_t)d] = codes(*w.after[d])[(size_t)lens[i] + (size_t)d];
            push(p.work, FileStair(lens[i], i));
        }
    }
    // the planned staircase becomes the state's: the stairs that reads of the batch left keep their codes from now on
    void adopt_host(std::vector<FileStair> &&work, const uint8_t *bases, const int64_t *offsets, int32_t n)
    {
        for (FileStair &s : work)
            if (s.read >= 0) {
                const uint8_t *c = bases + offsets[s.read];
                s.codes = std::make_shared<const std::vector<uint8_t>>(c, c + s.L);
                s.read = -1;
            }
        stairs = std::move(work); reads_seen += n; kind = HOST_FED;
    }

    // ---- the device feed: lengths only; an owner's 2-bit words are where words(owner) says ----
    // Seg = { words, first entry in the batch's tail, first position, owner's L, r, N } and After = { words of the owners of L, L + 1 } are
    // FoSeg and FoAfter of file_order.hip.inc, which this header cannot name.
    template <typename Seg, typename After, typename Words>
    void plan_device(const int32_t *lens, int32_t n, Words words, std::vector<FileStair> &work, std::vector<Seg> &segs,
                     std::vector<int64_t> &tail_off, std::vector<After> &own) const
    {
        work = stairs; segs.clear();
        tail_off.assign((size_t)n + 1, 0); own.assign((size_t)n, After{ { nullptr, nullptr } });
        FileWalk w;
        int64_t t = 0;
        for (int32_t i = 0; i < n; i++) {
            walk(work, lens[i], w);
            for (const FileWalk::Seg &s : w.segs) {
                segs.push_back(Seg{ words(*s.owner), t, (int32_t)s.p0, s.owner->L, s.owner->r, (int32_t)s.owner->N });
                t += s.count;
            }
            tail_off[(size_t)i + 1] = t;
            for (int d = 0; d < 2; d++)
                if (w.after[d]) own[(size_t)i].w[d] = words(*w.after[d]);
            push(work, FileStair(lens[i], i));
        }
    }
    // Of a planned staircase: the stairs of the state that survive (a prefix of it and of d_store), the words they occupy, and the words
    // the new stairs need behind them.
    struct Survivors { size_t kept; int64_t top, fresh; };
    static Survivors survivors(const std::vector<FileStair> &work)
    {
        Survivors s = { 0, 0, 0 };
        while (s.kept < work.size() && work[s.kept].read < 0) s.kept++;
        if (s.kept) s.top = work[s.kept - 1].woff + mtr_packed_words(work[s.kept - 1].L);
        for (size_t k = s.kept; k < work.size(); k++) s.fresh += mtr_packed_words(work[k].L);
        return s;
    }
};
