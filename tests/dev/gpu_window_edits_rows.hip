// gpu_window_edits_rows.hip — mtr_k_we_rows on the device against we_rows on the host, one window at a time: every carried field, the end, and every
// stored word (the bits of columns below W: the unrolled form also fills the bucket's columns beyond W, which nobody reads).  A program of its
// own, outside the library: it found that the unrolled register form of <32, narrow> and <16, wide> computes wrong rows with the row's stores in
// the loop, and a later session can use it to look for the cause - put WeRowRegs back for those two in window_edits.hip.inc,
// build, run.  One lane runs; the other 63 return, as the last group of a bin does.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fno-fast-math -mllvm -sink-insts-to-avoid-spills -mllvm -disable-machine-licm \
//         -Imtr_amd/csrc -Iinclude -o gpu_window_edits_rows tests/dev/gpu_window_edits_rows.hip      (the library's flags: mtr_amd/build.py)
//   ./gpu_window_edits_rows          prints one line per window and the differing words; exit 0 when all agree, 1 when one differs, 2 on a HIP error
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include <string>
#include "mtr_common.h"
#include "window_edits.hip.inc"
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e_), __LINE__); return 2; } } while (0)
static WsStruct pack(const std::vector<std::string> &ms)
{
    WsStruct st = { 0, 0, 0, 0, 0, (int32_t)ms.size() };
    int c = 0;
    for (size_t s = 0; s < ms.size(); s++) {
        st.first |= 1u << c;
        for (char ch : ms[s]) { uint64_t b = ch == 'A' ? 0 : ch == 'C' ? 1 : ch == 'G' ? 2 : 3; st.mot |= b << (2 * c); st.seg |= (uint64_t)s << (2 * c); c++; }
        st.last |= 1u << (c - 1);
    }
    st.W = c;
    return st;
}
template <int UB, bool WIDE> static int one(const std::vector<std::string> &ms, const std::string &win)
{
    const int n = (int)win.size(), NW = we_row_words(UB);
    const WsStruct st = pack(ms);
    std::vector<uint8_t> y(n + 16, 0);
    for (int i = 0; i < n; i++) y[i] = win[i] == 'A' ? 0 : win[i] == 'C' ? 1 : win[i] == 'G' ? 2 : 3;
    int64_t off[2] = { 0, n }; int32_t zero = 0, rows = n + 1; int64_t slot0 = 0;
    uint8_t *d_y; int64_t *d_off, *d_gslot; int32_t *d_ws, *d_tasks, *d_grows, *d_end; WsStruct *d_st; WsRaw *d_raw; uint32_t *d_scr;
    const size_t words = (size_t)(n + 1) * NW * 64;
    CK(hipMalloc(&d_y, n + 16)); CK(hipMalloc(&d_off, 16)); CK(hipMalloc(&d_gslot, 8)); CK(hipMalloc(&d_ws, 4)); CK(hipMalloc(&d_tasks, 4)); CK(hipMalloc(&d_grows, 4));
    CK(hipMalloc(&d_end, 4)); CK(hipMalloc(&d_st, sizeof st)); CK(hipMalloc(&d_raw, sizeof(WsRaw))); CK(hipMalloc(&d_scr, words * 4));
    CK(hipMemcpy(d_y, y.data(), n + 16, hipMemcpyHostToDevice)); CK(hipMemcpy(d_off, off, 16, hipMemcpyHostToDevice)); CK(hipMemcpy(d_gslot, &slot0, 8, hipMemcpyHostToDevice));
    CK(hipMemcpy(d_ws, &zero, 4, hipMemcpyHostToDevice)); CK(hipMemcpy(d_tasks, &zero, 4, hipMemcpyHostToDevice)); CK(hipMemcpy(d_grows, &rows, 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(d_st, &st, sizeof st, hipMemcpyHostToDevice)); CK(hipMemset(d_scr, 0xAB, words * 4)); CK(hipMemset(d_raw, 0xCD, sizeof(WsRaw))); CK(hipMemset(d_end, 0xEF, 4));
    WeArgs a{};
    a.ws.win_off = d_off; a.ws.win_bases = d_y; a.ws.win_struct = d_ws; a.ws.N = 1; a.ws.n_bases = n; a.ws.n_structs = 1; a.ws.structs = d_st; a.ws.tasks = d_tasks; a.ws.raw = d_raw;
    a.ws.G = 1; a.ws.MM = 1; a.ws.D = 1;
    a.bin_first[1] = a.bin_first[2] = a.bin_first[3] = a.bin_first[4] = a.bin_first[5] = 1;
    a.grp_first[1] = a.grp_first[2] = a.grp_first[3] = a.grp_first[4] = a.grp_first[5] = 1;
    a.grows = d_grows; a.gslot = d_gslot; a.scratch = d_scr; a.end_id = d_end;
    hipLaunchKernelGGL((mtr_k_we_rows<UB, WIDE>), dim3(1), dim3(64), 0, 0, a, 0u);
    CK(hipGetLastError()); CK(hipDeviceSynchronize());
    std::vector<uint32_t> scr(words); WsRaw raw; int32_t end;
    CK(hipMemcpy(scr.data(), d_scr, words * 4, hipMemcpyDeviceToHost)); CK(hipMemcpy(&raw, d_raw, sizeof raw, hipMemcpyDeviceToHost)); CK(hipMemcpy(&end, d_end, 4, hipMemcpyDeviceToHost));
    // the host's
    std::vector<uint32_t> hrows((size_t)(n + 1) * NW);
    const uint8_t *at = y.data(); const int r = 0;
    uint32_t *hp = hrows.data();
    int hend = -1;
    std::vector<uint8_t> pad(n + 24, 0); memcpy(pad.data(), y.data(), n);
    const uint8_t *pp = pad.data();
    const WsRaw hraw = we_rows<UB, WIDE>([pp](int k) { uint64_t v; memcpy(&v, pp + 8 * k, 8); return v; }, [hp, NW](int i, const WeRow &rec) { for (int k = 0; k < NW; k++) hp[(size_t)i * NW + k] = we_pack(UB, rec, k); }, r, n, st, 1, 1, 1, hend);
    (void)at;
    printf("<%d,%d> n %d W %d: device score %d end %d entry %llx copies %llx matches %llx | host score %d end %d entry %llx copies %llx matches %llx\n", UB, (int)WIDE, n, st.W, raw.score, end,
           (unsigned long long)raw.entry, (unsigned long long)raw.copies, (unsigned long long)raw.matches, hraw.score, hend, (unsigned long long)hraw.entry, (unsigned long long)hraw.copies, (unsigned long long)hraw.matches);
    int shown = 0;
    for (int i = 0; i <= n; i++) for (int k = 0; k < NW; k++) {
        const uint64_t kinds_mask = st.W >= 32 ? ~0ull : ((uint64_t)1 << (2 * st.W)) - 1;          // the columns below W
        const uint32_t mask = UB <= 8 ? ((uint32_t)kinds_mask & 0xffffu) | 0xffff0000u : k == 0 ? (uint32_t)kinds_mask : (UB > 16 && k == 1) ? (uint32_t)(kinds_mask >> 32) : ~0u;
        const uint32_t dv = scr[((size_t)i * NW + k) * 64] & mask, hv = hrows[(size_t)i * NW + k] & mask;
        if (dv != hv && shown++ < 12) printf("   row %d word %d: device %08x host %08x\n", i, k, dv, hv);
    }
    printf("   %d differing words of %d\n", shown, (n + 1) * NW);
    return shown > 0 || raw.score != hraw.score || end != hend || raw.entry != hraw.entry || raw.copies != hraw.copies || raw.matches != hraw.matches ? 1 : 0;
}
int main()
{
    int worst = 0;
    if (int rc = one<16, true>({ "GCGG", "CACA", "GA", "CAGCCG" }, "GCGGGCCGCAGATAGCATTAAATTTGACGCAAG")) worst = rc > worst ? rc : worst;
    if (int rc = one<32, false>({ "GGAGCCCAGAACCCAAA" }, "ATAGTACCC")) worst = rc > worst ? rc : worst;
    if (int rc = one<16, false>({ "GGAGCCCAGAACCCA" }, "ATAGTACCCGGAGCCC")) worst = rc > worst ? rc : worst;
    if (int rc = one<16, true>({ "CAG", "CAACAG", "CCG", "T" }, "CAGCAGCAACAGCCGCCGTCAG")) worst = rc > worst ? rc : worst;
    if (int rc = one<32, false>({ "GGAGCCCAGAACCCAAA" }, "ATAGTACCCGGAGCCCAGAACCAAAGG")) worst = rc > worst ? rc : worst;
    if (int rc = one<32, false>({ "GGAGCCCAGAACCCAAAGGAGCCCAGAACC", "CT" }, "GGAGCCCAGAACCCAAAGGAGCCCAGAACCCTCTGGAGCCAGAACCCAAAGGAGCCCAGAACCCT")) worst = rc > worst ? rc : worst;
    if (int rc = one<8, true>({ "CA", "G", "TC", "AAG" }, "CACAGTCTCAAGAAGCAGTC")) worst = rc > worst ? rc : worst;
    if (int rc = one<8, false>({ "CAG", "CCG" }, "CAGCAGCAACAGCCGCTGCCG")) worst = rc > worst ? rc : worst;
    return worst;
}
