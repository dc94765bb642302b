// Exact sums of doubles on the device, shared by mst_trans.hip and mst_trans_genome.hip.
//
// Every double is split into 32-bit pieces of a fixed-point number of 2112 bits (2^-1074 .. 2^1038) and the pieces are added
// as integers -- per workgroup in LDS, then one 64-bit integer atomic per piece and workgroup.  Integer addition is
// associative, so a sum is bit-identical under any permutation of the addends and any launch geometry; the one rounding per sum
// happens when the fixed-point total is converted back to a double.  No float atomics.
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>

namespace mst_exact {

constexpr int kLimbs = 66;              // 66 x 32 bits from 2^-1074: a 53-bit mantissa at the top exponent, with carry room
constexpr int kSumWords = kLimbs + 2;   // per sum: limbs, then {count, non-finite records}

// a += v as fixed-point pieces into lds[kLimbs] (two's complement per 64-bit word); returns false for a non-finite v
__device__ __forceinline__ bool add_exact(double v, unsigned long long *lds) {
    const unsigned long long bits = (unsigned long long)__double_as_longlong(v);
    const int ef = (int)((bits >> 52) & 0x7FF);
    if (ef == 0x7FF) return false;
    unsigned long long m = bits & ((1ull << 52) - 1);
    int p = 0;                                           // v = m * 2^(p - 1074)
    if (ef) {
        m |= 1ull << 52;
        p = ef - 1;
    }
    if (m == 0) return true;
    const bool neg = bits >> 63;
    const int L = p >> 5, s = p & 31;
    const unsigned long long lo = (m & 0xFFFFFFFFull) << s, hi = (m >> 32) << s;   // < 2^63, < 2^52
    const unsigned long long mid = (lo >> 32) + (hi & 0xFFFFFFFFull);
    const unsigned long long part[3] = {lo & 0xFFFFFFFFull, mid & 0xFFFFFFFFull, (hi >> 32) + (mid >> 32)};   // each < 2^32
#pragma unroll
    for (int k = 0; k < 3; ++k)
        if (part[k]) atomicAdd(&lds[L + k], neg ? (unsigned long long)(-(long long)part[k]) : part[k]);
    return true;
}

// the fixed-point total of words[0, kLimbs) (signed 64-bit words of weight 2^(32 i - 1074)) as a double, rounded ONCE to
// nearest-even: carries propagated, then the top 53 bits of the magnitude as an integer, a guard bit and a sticky bit OR-ed
// from every digit below, the rounding in integer arithmetic and one exact ldexp.  A magnitude of at most 53 bits (every
// subnormal total among them) is exact as it is.
__device__ inline double exact_to_double(const unsigned long long *words, long long *w /* LDS [kLimbs + 1] */) {
    long long carry = 0;
    for (int i = 0; i < kLimbs; ++i) {
        const long long t = (long long)words[i] + carry;          // |t| < 2^63 while fewer than 2^31 records were added
        long long d = t & 0xFFFFFFFFLL;
        carry = (t - d) >> 32;
        w[i] = d;
    }
    w[kLimbs] = carry;
    bool neg = w[kLimbs] < 0;
    if (neg) {                                                    // negate the two's complement number digit by digit
        long long c = 1;
        for (int i = 0; i <= kLimbs; ++i) {
            const long long t = ((~w[i]) & 0xFFFFFFFFLL) + c;
            w[i] = t & 0xFFFFFFFFLL;
            c = t >> 32;
        }
    }
    int top = kLimbs;
    while (top >= 0 && w[top] == 0) --top;
    if (top < 0) return 0.0;
    const int hb = 64 - __clzll((unsigned long long)w[top]);      // bits of the top digit, 1 .. 32
    const int nb = 32 * top + hb;                                 // bits of the magnitude
    double r;
    if (nb <= 53) {
        const unsigned long long m = ((unsigned long long)(top ? w[1] : 0) << 32) | (unsigned long long)w[0];
        r = ldexp((double)m, -1074);
    } else {
        // acc = the two top digits (hb + 32 bits, top >= 1); a top digit narrower than 22 bits takes the rest from the third
        const unsigned long long acc = ((unsigned long long)w[top] << 32) | (unsigned long long)w[top - 1];
        unsigned long long m, guard, sticky;
        int below;                                                // digits [0, below) lie under the guard bit entirely
        if (hb >= 22) {
            const int drop = hb + 32 - 53;                        // 1 .. 12 bits of acc under the mantissa
            m = acc >> drop;
            guard = (acc >> (drop - 1)) & 1ull;
            sticky = acc & ((1ull << (drop - 1)) - 1ull);
            below = top - 1;
        } else {
            const int need = 53 - (hb + 32);                      // 0 .. 20 bits of the third digit (top >= 2 here)
            const unsigned long long d = (unsigned long long)w[top - 2];
            m = (acc << need) | (d >> (32 - need));
            guard = (d >> (31 - need)) & 1ull;
            sticky = d & ((1ull << (31 - need)) - 1ull);
            below = top - 2;
        }
        for (int i = 0; i < below; ++i) sticky |= (unsigned long long)w[i];
        if (guard && (sticky || (m & 1ull))) ++m;                 // 2^53 at most: still exact as a double
        r = ldexp((double)m, nb - 53 - 1074);
    }
    return neg ? -r : r;
}

}  // namespace mst_exact
