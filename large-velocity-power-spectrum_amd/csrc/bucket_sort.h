// Two-level LDS bucket sort of particle records by a 32- or 64-bit key: the kernels and their geometry, once.
// Shared by the deposit (deposit.hip: key = bucket * cells + cell-in-bucket, buckets are bricks or z-pass pencils) and the NN
// cell list (nn.hip: key = a cell's linear index, cells = 1, so bucket = key).  The drivers stay with their users.
//
// What rank -> scan -> scatter with one global atomic per particle gives (records grouped by bucket + start[nbuckets + 1]),
// without that atomic (memory-side atomics cap such a pass at ~2.4e10 particles/s) and without random record-sized writes:
//   level 1: chunks of SORT_THREADS * ITEMS particles; per-chunk LDS histogram over coarse groups of 2^gshift consecutive
//            buckets -> table[group][chunk] -> exclusive scan (scan.h) -> each chunk ranks its particles in LDS, stages its
//            records in LDS in group order and streams {relative key, payload[C]} into its own contiguous run of every group
//   level 2: one workgroup per group: LDS histogram over the group's buckets, LDS scan (-> start[]), second sweep places
//            the record at its final slot
// Slots inside one bucket come out in no particular order (as with atomic ranks).
//
// What a user supplies:
//   key_of   functor  K operator()(long long i): the particle's full key, sort_invalid<K>() for "nowhere" (skipped throughout)
//   Payload  functor with  static constexpr int C  and  load(long long i, float val[C]): the C payload words of particle i
//   ITEMS    particles per thread of the level-1 kernels (the chunk and therefore nchunks follow from it)
//   KEEP_LOC whether the final record keeps the cell-in-bucket word: {loc, payload[C]}, or payload[4] alone as one 16-byte store
#pragma once
#include <hip/hip_runtime.h>

namespace {

#ifndef VPS_SORT_THREADS
#define VPS_SORT_THREADS 1024
#endif
constexpr int SORT_THREADS = VPS_SORT_THREADS;   // level 1: chunk = SORT_THREADS * ITEMS particles
constexpr int FINE_THREADS = 1024;               // level 2: one big workgroup per group
constexpr unsigned SORT_INVALID = 0xffffffffu;
// words per level-1 record {key, payload[C]}.  (Padding the 5-word record of C = 4 to an aligned 32-byte sector was
// measured: the level-1 scatter gains 10 %, level 2 loses 50 % to the extra bytes.)
__host__ __device__ constexpr int sort_rec1_words(int C) { return C + 1; }

struct SortGeom {
  int gshift, ngroups;     // buckets per group = 1 << gshift
  int cshift;              // log2(cells) when cells is a power of two, else -1
  unsigned cells;
  long long nbuckets, nchunks;
};

// Keys.  The full key of a particle is bucket * cells + cell-in-bucket: K = unsigned while that fits 32 bits, unsigned long
// long beyond (C4 on one GPU: 2^19 pencils x 2^14 cells).  It only lives in the keys[] array between the level-1 histogram
// and the level-1 scatter; the level-1 RECORD carries the key relative to its group's first bucket (< 2^gshift * cells),
// which is all level 2 -- one workgroup per group -- needs, and always 32 bits.
template <typename K>
__device__ __forceinline__ constexpr K sort_invalid() { return (K)~(K)0; }

template <typename K>
__device__ __forceinline__ unsigned sort_bucket_of(K key, const SortGeom& g) {
  return (unsigned)(g.cshift >= 0 ? (key >> g.cshift) : (key / g.cells));
}

// dynamic LDS of the three kernels
inline size_t sort_hist_lds(const SortGeom& g) { return sizeof(unsigned) * (size_t)g.ngroups; }
inline size_t sort_staged_lds(const SortGeom& g, int C, int items) {
  return sizeof(unsigned) * (2 * (size_t)g.ngroups + SORT_THREADS / 64 + (size_t)SORT_THREADS * items * (1 + sort_rec1_words(C)));
}
inline size_t sort_fine_lds(const SortGeom& g) { return sizeof(unsigned) * (((size_t)1 << g.gshift) + FINE_THREADS / 64); }

// Level-1 histogram.  keys != NULL: the keys are kept for the scatter (NULL when key_of reads that very array).
template <int ITEMS, typename K, typename KeyOf>
__global__ void __launch_bounds__(SORT_THREADS)
    sort_hist_kernel(KeyOf key_of, long long np, SortGeom g, K* __restrict__ keys, unsigned* __restrict__ table) {
  extern __shared__ unsigned sort_lds[];
  for (int i = threadIdx.x; i < g.ngroups; i += SORT_THREADS) sort_lds[i] = 0;
  __syncthreads();
  const long long base = (long long)blockIdx.x * (SORT_THREADS * ITEMS);
#pragma unroll 4
  for (int k = 0; k < ITEMS; ++k) {
    const long long i = base + (long long)k * SORT_THREADS + threadIdx.x;
    if (i < np) {
      const K key = key_of(i);
      if (key != sort_invalid<K>()) atomicAdd(&sort_lds[sort_bucket_of<K>(key, g) >> g.gshift], 1u);
      if (keys) keys[i] = key;
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < g.ngroups; i += SORT_THREADS)
    table[(long long)i * g.nchunks + blockIdx.x] = sort_lds[i];
}

// Level-1 scatter without the LDS staging: every record goes straight to its slot (option sort_staged = 0, or a group table
// the staged kernel's LDS cannot hold).
template <int ITEMS, typename K, typename Payload>
__global__ void __launch_bounds__(SORT_THREADS)
    sort_scatter_kernel(const K* __restrict__ keys, Payload pay, long long np, SortGeom g,
                        const unsigned* __restrict__ table_start, unsigned* __restrict__ rec1) {
  constexpr int C = Payload::C;
  extern __shared__ unsigned sort_lds[];
  for (int i = threadIdx.x; i < g.ngroups; i += SORT_THREADS)
    sort_lds[i] = table_start[(long long)i * g.nchunks + blockIdx.x];
  __syncthreads();
  const long long base = (long long)blockIdx.x * (SORT_THREADS * ITEMS);
#pragma unroll 4
  for (int k = 0; k < ITEMS; ++k) {
    const long long i = base + (long long)k * SORT_THREADS + threadIdx.x;
    if (i >= np) continue;
    const K key = keys[i];
    if (key == sort_invalid<K>()) continue;
    float val[C];
    pay.load(i, val);
    const unsigned grp = sort_bucket_of<K>(key, g) >> g.gshift;
    const unsigned slot = atomicAdd(&sort_lds[grp], 1u);
    constexpr int W = sort_rec1_words(C);
    unsigned w[W];
    w[0] = (unsigned)(key - (K)((unsigned long long)grp << g.gshift) * g.cells);   // relative to the group's first bucket
#pragma unroll
    for (int c = 0; c < C; ++c) w[1 + c] = __float_as_uint(val[c]);
    unsigned* rec = rec1 + (size_t)slot * W;
    if constexpr (W == 2) {
      *reinterpret_cast<uint2*>(rec) = make_uint2(w[0], w[1]);
    } else if constexpr (W == 4) {
      *reinterpret_cast<uint4*>(rec) = make_uint4(w[0], w[1], w[2], w[3]);
    } else {
#pragma unroll
      for (int c = 0; c < W; ++c) rec[c] = w[c];
    }
  }
}

// Exclusive scan of the LDS array a[0..n), n <= 4 * NT, in place; returns the total.
// `scratch` holds NT/64 words.  All NT threads of the workgroup must call it.
template <int NT>
__device__ __forceinline__ unsigned block_exclusive_scan(unsigned* a, int n, unsigned* scratch) {
  const int per = (n + NT - 1) / NT;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  unsigned v[4], mine = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int idx = tid * per + k;
    v[k] = (k < per && idx < n) ? a[idx] : 0u;
    mine += v[k];
  }
  unsigned inc = mine;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const unsigned up = __shfl_up(inc, off, 64);
    if (lane >= off) inc += up;
  }
  if (lane == 63) scratch[wave] = inc;
  __syncthreads();
  unsigned before = 0, total = 0;
#pragma unroll
  for (int w = 0; w < NT / 64; ++w) {
    const unsigned t = scratch[w];
    if (w < wave) before += t;
    total += t;
  }
  unsigned run = before + inc - mine;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int idx = tid * per + k;
    if (k < per && idx < n) {
      a[idx] = run;
      run += v[k];
    }
  }
  __syncthreads();
  return total;
}

// Level-1 scatter, LDS-staged: the chunk's records are first placed in LDS in group order, then
// streamed out word by word, so each (chunk, group) run leaves the CU as contiguous stores instead
// of 64 scattered dwords per instruction.  Consecutive chunks own adjacent runs of every group:
// they are dealt to the SAME XCD (blockIdx % 8, speed only) so that its L2 can merge the partly
// written lines at run boundaries.
template <int ITEMS, typename K, typename Payload>
__global__ void __launch_bounds__(SORT_THREADS)
    sort_scatter_staged_kernel(const K* __restrict__ keys, Payload pay, long long np, SortGeom g,
                               const unsigned* __restrict__ table_start, unsigned* __restrict__ rec1) {
  constexpr int C = Payload::C;
  constexpr int W = sort_rec1_words(C);
  constexpr int CHUNK = SORT_THREADS * ITEMS;
  extern __shared__ unsigned sort_lds[];
  unsigned* gbase = sort_lds;                        // [ngroups] first global slot of this chunk's run
  unsigned* lstart = gbase + g.ngroups;              // [ngroups] counts, then local exclusive starts
  unsigned* scratch = lstart + g.ngroups;            // [SORT_THREADS / 64]
  unsigned* gdest = scratch + SORT_THREADS / 64;     // [CHUNK] global slot of staged record p
  unsigned* stage = gdest + CHUNK;                   // [CHUNK * W]
  const long long per_xcd = (g.nchunks + 7) / 8;
  const long long chunk = (long long)(blockIdx.x % 8) * per_xcd + blockIdx.x / 8;
  if (chunk >= g.nchunks) return;
  for (int i = threadIdx.x; i < g.ngroups; i += SORT_THREADS) {
    gbase[i] = table_start[(long long)i * g.nchunks + chunk];
    lstart[i] = 0;
  }
  __syncthreads();
  const long long base = chunk * CHUNK;
  K key[ITEMS];
  unsigned grp[ITEMS], rk[ITEMS];
  float val[ITEMS][C];
#pragma unroll
  for (int k = 0; k < ITEMS; ++k) {
    const long long i = base + (long long)k * SORT_THREADS + threadIdx.x;
    key[k] = (i < np) ? keys[i] : sort_invalid<K>();
    if (key[k] != sort_invalid<K>()) pay.load(i, val[k]);
  }
#pragma unroll
  for (int k = 0; k < ITEMS; ++k) {
    if (key[k] != sort_invalid<K>()) {
      grp[k] = sort_bucket_of<K>(key[k], g) >> g.gshift;
      rk[k] = atomicAdd(&lstart[grp[k]], 1u);
    }
  }
  __syncthreads();
  const unsigned total = block_exclusive_scan<SORT_THREADS>(lstart, g.ngroups, scratch);
#pragma unroll
  for (int k = 0; k < ITEMS; ++k) {
    if (key[k] != sort_invalid<K>()) {
      const unsigned p = lstart[grp[k]] + rk[k];
      gdest[p] = gbase[grp[k]] + rk[k];
      stage[p * W] = (unsigned)(key[k] - (K)((unsigned long long)grp[k] << g.gshift) * g.cells);   // relative to the group's first bucket
#pragma unroll
      for (int c = 0; c < C; ++c) stage[p * W + 1 + c] = __float_as_uint(val[k][c]);
    }
  }
  __syncthreads();
  for (unsigned t = threadIdx.x; t < total * W; t += SORT_THREADS) {
    const unsigned rec = t / W, wd = t - rec * W;
    rec1[(size_t)gdest[rec] * W + wd] = stage[t];
  }
}

// Level 2.  KEEP_LOC: final records {cell-in-bucket, payload[C]} (the deposit); else payload[4] alone, 16-byte aligned and
// written with one 16-byte store (the NN cell list: a cell is a bucket, and the searches load a record as one float4).
template <int C, bool KEEP_LOC>
__global__ void __launch_bounds__(FINE_THREADS)
    sort_fine_kernel(const unsigned* __restrict__ rec1, SortGeom g, const unsigned* __restrict__ table_start,
                     unsigned* __restrict__ start, unsigned* __restrict__ records) {
  static_assert(KEEP_LOC || C == 4, "a final record without its cell-in-bucket word is one 16-byte store");
  constexpr int W = sort_rec1_words(C);
  extern __shared__ unsigned sort_lds[];          // [G] counts -> cursors, then scan scratch
  const int G = 1 << g.gshift;
  unsigned* cur = sort_lds;
  unsigned* scratch = sort_lds + G;
  const int grp = blockIdx.x;
  const unsigned gs = table_start[(long long)grp * g.nchunks];
  const unsigned ge = table_start[(long long)(grp + 1) * g.nchunks];   // [ngroups*nchunks] = total
  for (int i = threadIdx.x; i < G; i += FINE_THREADS) cur[i] = 0;
  __syncthreads();
  constexpr int U = 4;   // loads of U strides are issued together: the sweeps are latency bound otherwise
  // The second sweep reads the level-1 records with streaming loads: they are dead after it, and what
  // should stay in the caches are the final records it writes (the accumulation kernel reads them next:
  // pencil kernel -10 %).  The first sweep keeps plain loads so that the second finds the lines.
  // Streaming hints on the level-1 scatter itself cost 35 %.
  for (unsigned j0 = gs + threadIdx.x; j0 < ge; j0 += U * FINE_THREADS) {
    unsigned key[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const unsigned j = j0 + u * FINE_THREADS;
      key[u] = j < ge ? rec1[(size_t)j * W] : SORT_INVALID;
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (key[u] != SORT_INVALID) atomicAdd(&cur[sort_bucket_of<unsigned>(key[u], g) & (G - 1)], 1u);   // (keys relative to the group)
  }
  __syncthreads();
  // exclusive scan of the G counters, 4 * FINE_THREADS at a time (one round up to G = 4096, eight at 32768)
  unsigned carry = 0;
  for (int c0 = 0; c0 < G; c0 += 4 * FINE_THREADS) {
    const int n = min(4 * FINE_THREADS, G - c0);
    const unsigned tot = block_exclusive_scan<FINE_THREADS>(cur + c0, n, scratch);
    for (int f = threadIdx.x; f < n; f += FINE_THREADS) {
      const unsigned at = gs + carry + cur[c0 + f];
      cur[c0 + f] = at;
      const long long bucket = (long long)grp * G + c0 + f;
      if (bucket < g.nbuckets) start[bucket] = at;
    }
    carry += tot;
    __syncthreads();
  }
  if (grp == g.ngroups - 1 && threadIdx.x == 0) start[g.nbuckets] = ge;
  for (unsigned j0 = gs + threadIdx.x; j0 < ge; j0 += U * FINE_THREADS) {
    unsigned r[U][W];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const unsigned j = j0 + u * FINE_THREADS;
      r[u][0] = SORT_INVALID;
      if (j < ge) {
        const unsigned* src = rec1 + (size_t)j * W;
#pragma unroll
        for (int c = 0; c < W; ++c) r[u][c] = __builtin_nontemporal_load(&src[c]);
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (r[u][0] == SORT_INVALID) continue;
      const unsigned bucket = sort_bucket_of<unsigned>(r[u][0], g);
      const size_t slot = atomicAdd(&cur[bucket & (G - 1)], 1u);
      if constexpr (KEEP_LOC) {
        unsigned* dst = records + slot * W;
        dst[0] = r[u][0] - bucket * g.cells;
#pragma unroll
        for (int c = 1; c < W; ++c) dst[c] = r[u][c];
      } else {
        reinterpret_cast<uint4*>(records)[slot] = make_uint4(r[u][1], r[u][2], r[u][3], r[u][4]);
      }
    }
  }
}

}  // namespace
