// Development aid: can a DP wavefront (128 VGPRs, little LDS) enter a CU that already holds sixteen wavefronts of an arena kernel (about 10 KB of LDS each)?
// Two kernels with the footprints in question spin on a clock; A goes out on one stream as 4 096 one-wavefront workgroups (16 per CU), B on a second stream
// right behind it.  Every wavefront records its CU (XCC_ID + HW_ID), its start and its end on the constant 100 MHz clock (the same on every CU), and the
// host counts, per CU, the wavefronts of B that started while sixteen of A were resident there.  Registers: __launch_bounds__ sets the budget and a clobber
// of the highest register makes the allocation; LDS: a static array.  The table answers what arithmetic cannot: the LDS allocation granule and whether
// anything but registers and LDS caps a CU at sixteen of these wavefronts.
//   hipcc --offload-arch=gfx950 -O2 -o coresidency_probe coresidency_probe.hip && ./coresidency_probe
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <map>
#include <vector>

#define N_WAVES 4096
struct Stamp { unsigned cu; unsigned pad; unsigned long long t0, t1; };

#define GETREG(id) __builtin_amdgcn_s_getreg((31 << 11) | (0 << 6) | (id))        // the whole 32-bit register
template <int VGPRS, int LDS_BYTES>
__global__ __launch_bounds__(64, 512 / VGPRS) void k_spin(Stamp *out, int n, unsigned long long ticks)
{
    __shared__ int s_pad[LDS_BYTES / 4];
    const unsigned long long t0 = wall_clock64();
    if constexpr (VGPRS == 88) asm volatile("; v87 taken" ::: "v87");
    else if constexpr (VGPRS == 96) asm volatile("; v95 taken" ::: "v95");
    else if constexpr (VGPRS == 112) asm volatile("; v111 taken" ::: "v111");
    else asm volatile("; v127 taken" ::: "v127");
    ((volatile int *)s_pad)[threadIdx.x] = (int)t0;                              // (the array is used: it stays in the kernel's descriptor)
    unsigned long long t1 = t0;
    while (t1 - t0 < ticks) { __builtin_amdgcn_s_sleep(8); t1 = wall_clock64(); }
    if (threadIdx.x == 0 && (int)blockIdx.x < n) {
        const unsigned hw = GETREG(4), xcc = GETREG(20) & 15u;                   // HW_ID: cu 11:8, sh 12, se 15:13
        out[blockIdx.x].cu = (xcc << 8) | ((hw >> 8) & 0xffu);
        out[blockIdx.x].pad = ((volatile int *)s_pad)[0] == 0x7fffffff;
        out[blockIdx.x].t0 = t0; out[blockIdx.x].t1 = t1;
    }
}

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)
typedef void (*Kern)(Stamp *, int, unsigned long long);
struct Shape { const char *name; Kern k; };

static int run_pair(const Shape &A, const Shape &B, Stamp *dA, Stamp *dB, hipStream_t sA, hipStream_t sB)
{
    std::vector<Stamp> a(N_WAVES), b(N_WAVES);
    CHECK(hipMemset(dA, 0, sizeof(Stamp) * N_WAVES)); CHECK(hipMemset(dB, 0, sizeof(Stamp) * N_WAVES));
    CHECK(hipDeviceSynchronize());
    hipLaunchKernelGGL(A.k, dim3(N_WAVES), dim3(64), 0, sA, dA, N_WAVES, 400000ull);       // 4 ms of A
    hipLaunchKernelGGL(B.k, dim3(N_WAVES), dim3(64), 0, sB, dB, N_WAVES, 20000ull);        // 0.2 ms of B: 4 096 of them pass four at a time per CU in 0.8 ms
    CHECK(hipGetLastError());
    CHECK(hipDeviceSynchronize());
    CHECK(hipMemcpy(a.data(), dA, sizeof(Stamp) * N_WAVES, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(b.data(), dB, sizeof(Stamp) * N_WAVES, hipMemcpyDeviceToHost));
    std::map<unsigned, std::vector<const Stamp *>> onA;
    for (const Stamp &s : a) onA[s.cu].push_back(&s);
    int max_a = 0, beside16 = 0, beside_any = 0, max_b_beside = 0;
    for (auto &kv : onA) max_a = std::max<int>(max_a, (int)kv.second.size());
    std::map<unsigned, std::vector<std::pair<unsigned long long, int>>> ev;                 // per CU: B's starts and ends while sixteen of A were there
    for (const Stamp &s : b) {
        int n = 0;
        for (const Stamp *p : onA[s.cu]) if (p->t0 <= s.t0 && s.t0 < p->t1) n++;
        if (n > 0) beside_any++;
        if (n >= 16) { beside16++; ev[s.cu].push_back({ s.t0, +1 }); ev[s.cu].push_back({ s.t1, -1 }); }
    }
    for (auto &kv : ev) {
        std::sort(kv.second.begin(), kv.second.end());                                    // (an end sorts before a start at the same tick)
        int cur = 0;
        for (auto &e : kv.second) { cur += e.second; max_b_beside = std::max(max_b_beside, cur); }
    }
    hipFuncAttributes fa, fb;
    CHECK(hipFuncGetAttributes(&fa, (const void *)A.k)); CHECK(hipFuncGetAttributes(&fb, (const void *)B.k));
    printf("| %-14s | %3d | %6zu | %-14s | %3d | %6zu | %4zu | %3d | %5d | %5d | %2d |\n", A.name, fa.numRegs, fa.sharedSizeBytes, B.name, fb.numRegs, fb.sharedSizeBytes,
           onA.size(), max_a, beside_any, beside16, max_b_beside);
    return 0;
}

int main()
{
    const Shape A88 = { "88 + 10080 B", k_spin<88, 10080> }, A96 = { "96 + 10080 B", k_spin<96, 10080> }, A112 = { "112 + 10080 B", k_spin<112, 10080> },
                A96s = { "96 + 8960 B", k_spin<96, 8960> }, A96m = { "96 + 9600 B", k_spin<96, 9600> };
    const Shape B448 = { "128 + 448 B", k_spin<128, 448> }, B960 = { "128 + 960 B", k_spin<128, 960> }, B1536 = { "128 + 1536 B", k_spin<128, 1536> };
    Stamp *dA = nullptr, *dB = nullptr;
    CHECK(hipMalloc(&dA, sizeof(Stamp) * N_WAVES)); CHECK(hipMalloc(&dB, sizeof(Stamp) * N_WAVES));
    hipStream_t sA, sB;
    CHECK(hipStreamCreateWithFlags(&sA, hipStreamNonBlocking)); CHECK(hipStreamCreateWithFlags(&sB, hipStreamNonBlocking));
    printf("A: 4 096 one-wavefront workgroups spinning 4 ms; B: 4 096 spinning 0.2 ms, launched behind A on a second stream.\n");
    printf("| A (VGPRs + LDS) | regs | LDS | B (VGPRs + LDS) | regs | LDS | CUs | max A per CU | B started beside any A | B started beside 16 A on its CU | most B at once beside 16 A |\n");
    printf("|---|---|---|---|---|---|---|---|---|---|---|\n");
    const Shape *pairs[][2] = { { &A112, &B448 }, { &A88, &B448 }, { &A96, &B448 }, { &A96, &B960 }, { &A96, &B1536 }, { &A96m, &B448 }, { &A96m, &B960 }, { &A96s, &B960 }, { &A96s, &B1536 } };
    for (auto &p : pairs) if (run_pair(*p[0], *p[1], dA, dB, sA, sB)) return 1;
    (void)hipFree(dA); (void)hipFree(dB); (void)hipStreamDestroy(sA); (void)hipStreamDestroy(sB);
    return 0;
}
