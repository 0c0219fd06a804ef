// allele_split.h — the split of ONE locus' sorted supporting values into one or two alleles, as the functions the split kernel runs per lane
// (allele_call.hip.inc: mtr_k_allele_split).  Plain C++, nothing of HIP: the same functions compile into the gfx950 kernel and into a host
// program (tests/allele_split_check.cpp).
//
// The definition is include/mtr_hip.h's ("allele calls"): for the sorted values v[0 .. S) of a locus,
//   med(i, j)   = v[i + (j - i - 1) / 2], the lower median of the segment [i, j), i < j
//   sad(i, j)   = sum over t in [i, j) of |v[t] - med(i, j)|, as int64
//   a split k, 1 <= k < S, is admissible iff v[k - 1] < v[k], min(k, S - k) >= min_support, min(k, S - k) * 100 >= min_percent * S (int64)
//   and med(k, S) - med(0, k) >= min_sep; its cost is sad(0, k) + sad(k, S); the split taken has the smallest cost, the smallest k on a tie.
// sad comes in O(1) from the prefix sums pre[t] = v[0] + .. + v[t - 1] (pre[0] = 0, S + 1 entries, int64): with m the median's index and x =
// v[m], the members below m lie x - v[t] under it and the members from m on v[t] - x over it, so
//   sad(i, j) = x * (m - i) - (pre[m] - pre[i]) + (pre[j] - pre[m]) - x * (j - m).
// Values are 0 .. 2^31 - 1 and S <= 2^31 - 1: every product and every sum stays under 2^62.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ALS_HD static inline __host__ __device__ __attribute__((always_inline))
#else
#define ALS_HD static inline __attribute__((always_inline))
#endif

struct AlleleRule { int32_t min_support, min_percent, min_sep; };
struct AlleleSeg { int64_t sad; int32_t med; };                  // one segment: its sum of absolute deviations from its lower median, the median
struct AlleleSplit { int64_t cost; int64_t k; int32_t med[2]; }; // one split: cost2(k), k, med(0, k) and med(k, S); k = 0: none

#define ALS_NO_COST INT64_MAX

// the segment [i, j), i < j, of the sorted values v with their prefix sums pre
ALS_HD AlleleSeg allele_seg(const int32_t *v, const int64_t *pre, int64_t i, int64_t j)
{
    const int64_t m = i + (j - i - 1) / 2;
    const int64_t x = v[m];
    AlleleSeg s;
    s.med = (int32_t)x;
    s.sad = x * (m - i) - (pre[m] - pre[i]) + (pre[j] - pre[m]) - x * (j - m);
    return s;
}

// the split k of S values, 1 <= k < S: admissible by the rule?  then out is the split
ALS_HD bool allele_admissible(const int32_t *v, const int64_t *pre, int64_t S, int64_t k, const AlleleRule &r, AlleleSplit &out)
{
    if (!(v[k - 1] < v[k])) return false;
    const int64_t small = k < S - k ? k : S - k;
    if (small < (int64_t)r.min_support || small * 100 < (int64_t)r.min_percent * S) return false;
    const AlleleSeg lo = allele_seg(v, pre, 0, k), hi = allele_seg(v, pre, k, S);
    if ((int64_t)hi.med - (int64_t)lo.med < (int64_t)r.min_sep) return false;
    out.cost = lo.sad + hi.sad; out.k = k; out.med[0] = lo.med; out.med[1] = hi.med;
    return true;
}

// is the split a better than b?  the smaller cost, the smaller k on a tie; "none" (k = 0, ALS_NO_COST) loses to every split
ALS_HD bool allele_better(int64_t cost_a, int64_t k_a, int64_t cost_b, int64_t k_b)
{
    if (k_a == 0) return false;
    if (k_b == 0) return true;
    return cost_a < cost_b || (cost_a == cost_b && k_a < k_b);
}

ALS_HD AlleleSplit allele_no_split()
{
    AlleleSplit s;
    s.cost = ALS_NO_COST; s.k = 0; s.med[0] = s.med[1] = 0;
    return s;
}

// the best admissible split among k = first, first + step, ... below S (the kernel: one share per lane; the host: first = 1, step = 1)
ALS_HD AlleleSplit allele_best_split(const int32_t *v, const int64_t *pre, int64_t S, const AlleleRule &r, int64_t first, int64_t step)
{
    AlleleSplit best = allele_no_split(), s = best;
    for (int64_t k = first; k < S; k += step)
        if (allele_admissible(v, pre, S, k, r, s) && allele_better(s.cost, s.k, best.cost, best.k)) best = s;
    return best;
}
