// Helpers shared by the eligible-row selections (score_filtered.hip, score_grouped.hip, score_after.hip): order-preserving keys
// of fp32 and float64 scores, the bitonic sorts of maxima keys and of (key, row) entries, the padding row of the select stages.
#pragma once
#include <stdint.h>

#define FT_MAXSPLIT 16       // splits with maxima slots of their own
#define FT_KEY_NINF 0x007FFFFFu  // key of -inf: finite scores have larger keys, 0 = empty slot

__device__ __forceinline__ uint32_t ft_key(float x) {
  const uint32_t u = __float_as_uint(x);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ft_unkey(uint32_t u) { return __uint_as_float((u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u); }

// bitonic sort of n2 (power of two) keys in LDS, descending
__device__ __forceinline__ void ft_sort_u32(uint32_t *key, int n2, int tid, int nthr) {
  for (int size = 2; size <= n2; size <<= 1)
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      __syncthreads();
      for (int i = tid; i < (n2 >> 1); i += nthr) {
        const int lo = 2 * i - (i & (stride - 1)), hi = lo + stride;
        const bool desc = ((lo & size) == 0);
        const uint32_t x = key[lo], y = key[hi];
        if ((x < y) == desc) {
          key[lo] = y;
          key[hi] = x;
        }
      }
    }
  __syncthreads();
}

__device__ __forceinline__ unsigned long long ft_key64(double x) {
  const unsigned long long u = (unsigned long long)__double_as_longlong(x);
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double ft_unkey64(unsigned long long u) {
  return __longlong_as_double((long long)((u >> 63) ? (u & 0x7FFFFFFFFFFFFFFFull) : ~u));
}

#define FT_PAD_ROW 0x7FFFFFFF  // (padding entries: key 0 is below the key of every score, -inf included)

// bitonic sort of n2 (power of two) entries in LDS by (key descending, row ascending): the order of before()
__device__ __forceinline__ void ft_sort_entries(unsigned long long *skey, int *srow, int n2, int tid) {
  for (int size = 2; size <= n2; size <<= 1)
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      __syncthreads();
      for (int i = tid; i < (n2 >> 1); i += 256) {
        const int lo = 2 * i - (i & (stride - 1)), hi = lo + stride;
        const bool desc = ((lo & size) == 0);
        const unsigned long long x = skey[lo], y = skey[hi];
        const int rx = srow[lo], ry = srow[hi];
        const bool x_after_y = (x < y) || (x == y && rx > ry);
        if (x_after_y == desc) {
          skey[lo] = y;
          skey[hi] = x;
          srow[lo] = ry;
          srow[hi] = rx;
        }
      }
    }
  __syncthreads();
}
