// exp4.hip — the experiment-4 probe strand: R probes the table on S, then (keyed by the same
// R.k) the table on T; results are triples (r, s, t).
//
//   Ndu (nested tables, main_experiment4.cc:831-941): AlgNestJoinProbe(S) -> AlgNestJoinProbe(T)
//       -> AlgUnnestHt(T) -> AlgUnnestHt(S) -> AlgTop. The S matches stay nested until T also
//       matched ("deferred unnesting"), so R tuples that fail the second join never expand S.
//   Chj (chaining tables, main_experiment4.cc:943-1043): AlgHashJoinProbe(S) emits every (r,s)
//       pair, and each pair probes T (full chain walk, no early exit).
// Counters are the reference's CSV columns; with the GPU layouts they are closed forms per r:
//   Ndu: cmps as nested probes; unnest_1 += |T(k)|; unnest_2 = top += |S(k)|*|T(k)|
//   Chj: c_probe_rs += mS; cmp_rs += nS; cmp_rt += mS*nT (only if T's bucket is non-empty);
//        c_probe_rt = top += mS*mT
// Triples are enumerated for the checksums and, with HJ3D_PROBE_EMIT (the EMIT instantiations), written
// to the caller's buffer as {u32 r, s, t}; products above kInline2 are handed to whole workgroups (heavy
// queue), as in nested.hip.
// Write-out (one pass): word kResCursor of the result slot is a u64 output cursor. A unit of work
// reserves a contiguous slot range with ONE atomic add on it and writes its triples there: on the light
// path the lanes of a wave that are active at that point together (wave_reserve), on the heavy path
// the workgroup per queued item. Triples whose slot is >= out_cap are dropped; the cursor and c_top
// still count them. EMIT is a template parameter, so the counting kernels carry none of this.
#include "radix_seg.hpp"

namespace hj3d {
namespace {

constexpr int kItems = 2;
constexpr uint64_t kInline2 = 64;
constexpr int kF = 12;  // c_probe_rs, cmp_rs, c_probe_rt, cmp_rt, unnest_1, unnest_2, top, sum_a, sum_b, sum_c, sum_h, xor_h

constexpr int kResCursor = 12;  // result-slot word of the EMIT output cursor (words 0..11: hj3d_probe2_res)

struct Heavy2 {
  uint32_t r;   // probe row
  uint32_t ms;  // S side: nested main index, or the chaining hash
  uint32_t mt;  // T side: nested main index; chaining with EMIT: matching S entries
  uint32_t pad;  // chaining with EMIT: matching T entries
};

// Where the triples go. The counting kernels take the empty form.
template <bool EMIT>
struct Out {};
template <>
struct Out<true> {
  uint32_t* out;            // out_cap triples of 3 words
  uint64_t cap;
  unsigned long long* cur;  // res + kResCursor
};

typedef uint32_t u32x3 __attribute__((ext_vector_type(3)));
typedef u32x3 u32x3_a4 __attribute__((aligned(4)));  // a triple is 4-byte aligned only

__device__ __forceinline__ void store_triple(uint32_t* p, uint32_t r, uint32_t s, uint32_t t) {
  u32x3 v;
  v.x = r;
  v.y = s;
  v.z = t;
  __builtin_nontemporal_store(v, reinterpret_cast<u32x3_a4*>(p));
}

// Output slots for the n <= kInline2 triples of every lane ACTIVE HERE: one contiguous range, reserved
// with one atomic add by the first of them and split in lane order. Returns the range's first slot
// (wave-uniform) and in *pre this lane's offset into it. The prefix is taken bit by bit with ballots,
// which count active lanes only, so it holds for any active set (no shuffle reads a lane that is not
// here). *tot: the range's length (wave-uniform, <= 64 * kInline2).
__device__ __forceinline__ uint64_t wave_reserve(unsigned long long* cur, uint32_t n, uint32_t* pre, uint32_t* tot) {
  static_assert(kInline2 < 128, "wave_reserve splits n into 7 bits");
  uint32_t p = 0, t = 0;
#pragma unroll
  for (int b = 0; b < 7; ++b) {
    const uint64_t m = __ballot((n >> b) & 1u);
    p += __builtin_amdgcn_mbcnt_hi(uint32_t(m >> 32), __builtin_amdgcn_mbcnt_lo(uint32_t(m), 0u)) << b;
    t += uint32_t(__popcll(m)) << b;
  }
  *pre = p;
  *tot = t;
  const uint64_t act = __ballot(1);
  const uint32_t lane = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
  uint64_t base = 0;
  if (lane == uint32_t(__ffsll(static_cast<long long>(act)) - 1))
    base = atomicAdd(cur, static_cast<unsigned long long>(t));
  // (the first active lane is the one that added)
  const uint32_t lo = __builtin_amdgcn_readfirstlane(uint32_t(base)),
                 hi = __builtin_amdgcn_readfirstlane(uint32_t(base >> 32));
  return (uint64_t(hi) << 32) | lo;
}

// A contiguous slot range of n triples from slot `base`, of which the first `lim` fit the buffer;
// put(k, ...) writes the range's k-th triple. The counting kernels take the empty form.
template <bool EMIT>
struct Range {
  __device__ __forceinline__ Range(const Out<false>&, uint64_t, uint64_t) {}
  __device__ __forceinline__ void put(uint64_t, uint32_t, uint32_t, uint32_t) const {}
};
template <>
struct Range<true> {
  uint32_t* p;
  uint64_t lim;
  __device__ __forceinline__ Range(const Out<true>& o, uint64_t base, uint64_t n) {
    const uint64_t room = base < o.cap ? o.cap - base : 0;
    lim = room < n ? room : n;
    p = o.out + 3 * (lim ? base : 0);
  }
  __device__ __forceinline__ void put(uint64_t k, uint32_t r, uint32_t s, uint32_t t) const {
    if (k < lim) store_triple(p + 3 * k, r, s, t);
  }
};
// One lane's range on the light path (n <= kInline2), reserved by the wave's active lanes together.
template <bool EMIT>
struct LaneOut {
  __device__ __forceinline__ LaneOut(const Out<false>&, uint32_t) {}
  __device__ __forceinline__ void put(uint32_t, uint32_t, uint32_t) {}
};
template <>
struct LaneOut<true> {
  uint32_t* wp;   // the wave's range (wave-uniform, as is room)
  uint32_t room;  // triples of the wave's range that fit the buffer
  uint32_t k;     // this lane's next triple in the wave's range
  __device__ __forceinline__ LaneOut(const Out<true>& o, uint32_t n) {
    uint32_t tot;
    const uint64_t base = wave_reserve(o.cur, n, &k, &tot);
    const uint64_t left = base < o.cap ? o.cap - base : 0;
    room = left < tot ? uint32_t(left) : tot;
    wp = o.out + 3 * (room ? base : 0);
  }
  __device__ __forceinline__ void put(uint32_t r, uint32_t s, uint32_t t) {
    if (k < room) store_triple(wp + 3 * k, r, s, t);
    ++k;
  }
};

// One output triple: its row sums always (the unnest reads every sub row, as AlgUnnestHt::step,
// algebra.hh:510-541, produces every tuple), its hash only with HJ3D_PROBE_CHECKSUM (ck; the
// verification checksums, which the reference does not compute; two mix64 per triple).
__device__ __forceinline__ void add_triple(uint64_t (&a)[kF], uint32_t r, uint32_t s, uint32_t t, bool ck) {
  a[7] += r;
  a[8] += s;
  a[9] += t;
  if (ck) {
    const uint64_t h = triple_hash(r, s, t);
    a[10] += h;
    a[11] ^= h;
  }
}

struct NTab {  // nested table view
  const uint32_t* off;
  const uint4* mains;
  const uint32_t* sub;
  FastMod fm;
  uint32_t lo, nbl;
  // returns main index or kInvalid; adds the reference's comparison count to *cmps
  __device__ __forceinline__ uint32_t find(uint32_t h, uint64_t* cmps, uint4* M) const;
};

// Main record of hash h among M[s .. s+n) (one bucket), or kInvalid; adds the reference's
// comparison count (findMainNodeByOther, ht_nested.hh:354-382) to *cmps. M: HBM or LDS.
template <typename MT>
__device__ __forceinline__ uint32_t nfind(uint32_t h, const MT* M, uint32_t s, uint32_t n, uint64_t* cmps, uint4* F) {
  uint32_t found = kInvalid;
  for (uint32_t k = s; k < s + n; ++k) {
    const uint4 c = M[k];
    if (c.x == h) { found = k; *F = c; break; }
  }
  if (found == kInvalid) { *cmps += n; return kInvalid; }
  uint32_t before = 0;
  for (uint32_t k = s; k < s + n; ++k) before += M[k].y < F->y;
  *cmps += 1 + before;
  return found;
}

__device__ __forceinline__ uint32_t NTab::find(uint32_t h, uint64_t* cmps, uint4* M) const {
  const uint32_t b = fm.mod(h) - lo;
  if (b >= nbl) return kInvalid;
  const uint32_t s = off[b];
  return nfind(h, mains, s, off[b + 1] - s, cmps, M);
}

struct CTab {  // chaining table view
  const uint32_t* off;
  const uint2* ent;
  FastMod fm;
  uint32_t lo, nbl;
  __device__ __forceinline__ void range(uint32_t h, uint32_t* s, uint32_t* e) const {
    const uint32_t b = fm.mod(h) - lo;
    *s = 0;
    *e = 0;
    if (b < nbl) { *s = off[b]; *e = off[b + 1]; }
  }
};

// Triples of one light match (|S(k)| x |T(k)| <= kInline2): the sub rows are loaded in blocks
// of 8 into registers before they are combined, so a match costs one or two memory latencies
// instead of one per sub row. EMIT: the wave's active lanes reserve their slots together first.
template <bool EMIT>
__device__ __forceinline__ void light_triples(uint64_t (&a)[kF], uint32_t pr, const NTab& S, const NTab& T, uint32_t zs,
                                              uint32_t ws, uint32_t zt, uint32_t wt, bool ck, const Out<EMIT>& o) {
  // (EMIT: blocks of 4; with 8 the partitioned kernel, 128 VGPRs for its 1024 threads, spilled)
  constexpr uint32_t kB = EMIT ? 4 : 8;
  LaneOut<EMIT> w(o, ws * wt);
  for (uint32_t qb = 0; qb < wt; qb += kB) {
    uint32_t tv[kB];
#pragma unroll
    for (uint32_t u = 0; u < kB; ++u) tv[u] = qb + u < wt ? T.sub[zt + qb + u] : 0u;
    for (uint32_t pb = 0; pb < ws; pb += kB) {
      uint32_t sv[kB];
#pragma unroll
      for (uint32_t u = 0; u < kB; ++u) sv[u] = pb + u < ws ? S.sub[zs + pb + u] : 0u;
#pragma unroll
      for (uint32_t qu = 0; qu < kB; ++qu) {
        if (qb + qu >= wt) break;
#pragma unroll
        for (uint32_t pu = 0; pu < kB; ++pu)
          if (pb + pu < ws) {
            add_triple(a, pr, sv[pu], tv[qu], ck);
            w.put(pr, sv[pu], tv[qu]);
          }
      }
    }
  }
}

// Ndu for one probe tuple after its two lookups (ms / mt: global main indices or kInvalid).
template <bool EMIT>
__device__ __forceinline__ void ndu_tail(uint64_t (&a)[kF], uint32_t pr, const NTab& S, const NTab& T, uint32_t ms,
                                         const uint4& MS, uint32_t mt, const uint4& MT, Heavy2* __restrict__ heavy,
                                         uint64_t* __restrict__ nheavy, bool ck, const Out<EMIT>& o) {
  a[2] += 1;
  a[4] += MT.w;
  const uint64_t prod = uint64_t(MS.w) * MT.w;
  a[5] += prod;
  a[6] += prod;
  if (prod <= kInline2) {
    light_triples<EMIT>(a, pr, S, T, MS.z, MS.w, MT.z, MT.w, ck, o);
  } else {
    const uint64_t slot = atomicAdd(reinterpret_cast<unsigned long long*>(nheavy), 1ull);
    heavy[slot] = Heavy2{pr, ms, mt, 0};
  }
}

// AlgNestJoinProbe(S) -> AlgNestJoinProbe(T) -> unnest both, for one probe tuple (HBM tables).
template <bool EMIT>
__device__ __forceinline__ void ndu_probe(uint64_t (&a)[kF], uint32_t h, uint32_t pr, const NTab& S, const NTab& T,
                                          Heavy2* __restrict__ heavy, uint64_t* __restrict__ nheavy, bool ck,
                                          const Out<EMIT>& o) {
  uint4 MS, MT;
  const uint32_t ms = S.find(h, &a[1], &MS);
  if (ms == kInvalid) return;
  a[0] += 1;
  const uint32_t mt = T.find(h, &a[3], &MT);
  if (mt == kInvalid) return;
  ndu_tail<EMIT>(a, pr, S, T, ms, MS, mt, MT, heavy, nheavy, ck, o);
}

template <bool EMIT>
__global__ __launch_bounds__(kBlock) void k_ndu(RelView r, NTab S, NTab T, Heavy2* __restrict__ heavy,
                                                uint64_t* __restrict__ nheavy, uint64_t* __restrict__ res, bool ck,
                                                Out<EMIT> o) {
  uint64_t a[kF] = {0};
  for (uint64_t i = uint64_t(blockIdx.x) * kBlock + threadIdx.x; i < r.n; i += uint64_t(gridDim.x) * kBlock)
    ndu_probe<EMIT>(a, murmur32(r.key(i)), r.row(i), S, T, heavy, nheavy, ck, o);
  block_flush<kF, 1>(a, res);
}

// Partitioned Ndu (S and T tables with the same bucket function): the probe side is
// partitioned by bucket range (radix_partition_probe) and each partition's slices of BOTH
// tables (directories + main records) are staged in LDS; the lookups of both joins then run
// against LDS. FITS as in k_rp_probe_seg (false: the slices are read through L2).
template <bool FITS, bool EMIT>
__global__ __launch_bounds__(kJBlock) void k_ndu_seg(const uint2* __restrict__ region, const uint32_t* __restrict__ counts,
                                                     const uint32_t* __restrict__ seg, uint32_t G, uint32_t cap, NTab S,
                                                     NTab T, uint32_t W, uint32_t P, uint32_t splits, bool flat,
                                                     Heavy2* __restrict__ heavy, uint64_t* __restrict__ nheavy,
                                                     uint64_t* __restrict__ res, bool ck, Out<EMIT> o) {
  __shared__ uint32_t lds[kProbeLdsWords];
  const uint32_t p = blockIdx.x / splits, sp = blockIdx.x % splits;
  const uint32_t b0 = p * W;
  const uint32_t nbs = min(W, S.nbl - b0);
  const uint32_t s0 = S.off[b0], ns = S.off[b0 + nbs] - s0;
  const uint32_t t0 = T.off[b0], nt = T.off[b0 + nbs] - t0;
  const uint32_t dirw = (2 * nbs + 4) & ~3u;  // both directories, then 16-B aligned main records
  const bool fits = dirw + 4ull * (ns + nt) <= kProbeLdsWords;
  if (fits != FITS) return;
  uint32_t* ldS = lds;
  uint32_t* ldT = lds + nbs;
  uint4* lmS = reinterpret_cast<uint4*>(lds + dirw);
  uint4* lmT = lmS + ns;
  uint64_t a[kF] = {0};
  seg_walk(region, counts, seg, G, cap, P, p, splits, sp, flat,
           [&] {
             if (FITS) {
               stage_nested(S.off, S.mains, b0, nbs, s0, ns, ldS, lmS);
               stage_nested(T.off, T.mains, b0, nbs, t0, nt, ldT, lmT);
             }
           },
           [&](uint32_t h, uint32_t pr, uint64_t) {
             if (!FITS) {
               ndu_probe<EMIT>(a, h, pr, S, T, heavy, nheavy, ck, o);
               return;
             }
             const uint32_t bl = S.fm.mod(h) - S.lo - b0;
             uint4 MS, MT;
             const uint32_t ds = ldS[bl];
             const uint32_t ms = nfind(h, lmS, ds >> 16, ds & 0xFFFFu, &a[1], &MS);
             if (ms == kInvalid) return;
             a[0] += 1;
             const uint32_t dt = ldT[bl];
             const uint32_t mt = nfind(h, lmT, dt >> 16, dt & 0xFFFFu, &a[3], &MT);
             if (mt == kInvalid) return;
             ndu_tail<EMIT>(a, pr, S, T, s0 + ms, MS, t0 + mt, MT, heavy, nheavy, ck, o);
           });
  block_flush<kF, 1>(a, res);
}

// Overflow pairs of the partition (runs that did not fit their region), against the HBM tables.
template <bool EMIT>
__global__ __launch_bounds__(kBlock) void k_ndu_ovf(const uint2* __restrict__ ovf, const unsigned long long* __restrict__ novf,
                                                    NTab S, NTab T, Heavy2* __restrict__ heavy,
                                                    uint64_t* __restrict__ nheavy, uint64_t* __restrict__ res, bool ck,
                                                    Out<EMIT> o) {
  uint64_t a[kF] = {0};
  const uint64_t n = *novf;
  for (uint64_t j = uint64_t(blockIdx.x) * kBlock + threadIdx.x; j < n; j += uint64_t(gridDim.x) * kBlock)
    ndu_probe<EMIT>(a, ovf[j].x, ovf[j].y, S, T, heavy, nheavy, ck, o);
  block_flush<kF, 1>(a, res);
}

// The workgroup's slot range for one queued heavy item of n triples: one atomic add by thread 0,
// handed to the others through LDS (two words taken in turn by the item count `it`, so one barrier per
// item is enough). Called by all threads of the workgroup.
template <bool EMIT>
__device__ __forceinline__ uint64_t block_reserve(const Out<EMIT>& o, uint64_t n, uint32_t it) {
  if constexpr (EMIT) {
    __shared__ uint64_t sbase[2];
    if (threadIdx.x == 0) sbase[it & 1] = atomicAdd(o.cur, static_cast<unsigned long long>(n));
    __syncthreads();
    return sbase[it & 1];
  } else {
    return 0;
  }
}

// Heavy nested products: the workgroup's threads stride over the product; triple k of an item goes to
// the item's slot base + k (EMIT).
template <bool EMIT>
__global__ __launch_bounds__(kBlock) void k_ndu_heavy(NTab S, NTab T, const Heavy2* __restrict__ heavy,
                                                      const uint64_t* __restrict__ nheavy, uint64_t* __restrict__ res,
                                                      bool ck, Out<EMIT> o) {
  uint64_t a[kF] = {0};
  const uint64_t nh = *nheavy;
  uint32_t it = 0;
  for (uint64_t q = blockIdx.x; q < nh; q += gridDim.x, ++it) {
    const Heavy2 hv = heavy[q];
    const uint4 MS = S.mains[hv.ms], MT = T.mains[hv.mt];
    const uint64_t prod = uint64_t(MS.w) * MT.w;
    const Range<EMIT> w(o, block_reserve<EMIT>(o, prod, it), prod);
    for (uint64_t k = threadIdx.x; k < prod; k += kBlock) {
      const uint32_t tq = uint32_t(k / MS.w), sq = uint32_t(k % MS.w);
      const uint32_t sr = S.sub[MS.z + sq], tr = T.sub[MT.z + tq];
      add_triple(a, hv.r, sr, tr, ck);
      w.put(k, hv.r, sr, tr);
    }
  }
  block_flush<kF, 1>(a, res);
}

template <bool EMIT>
__global__ __launch_bounds__(kBlock) void k_chj(RelView r, CTab S, CTab T, Heavy2* __restrict__ heavy,
                                                uint64_t* __restrict__ nheavy, uint64_t* __restrict__ res, bool ck,
                                                Out<EMIT> o) {
  uint64_t a[kF] = {0};
  for (uint64_t i = uint64_t(blockIdx.x) * kBlock + threadIdx.x; i < r.n; i += uint64_t(gridDim.x) * kBlock) {
    const uint32_t h = murmur32(r.key(i));
    const uint32_t pr = r.row(i);
    uint32_t s0, s1, t0, t1;
    S.range(h, &s0, &s1);
    if (s0 == s1) continue;  // empty S bucket: no comparisons (algebra.hh:640-643)
    a[1] += s1 - s0;
    uint32_t mS = 0;
    for (uint32_t k = s0; k < s1; ++k) mS += S.ent[k].x == h;
    if (mS == 0) continue;
    a[0] += mS;
    T.range(h, &t0, &t1);
    if (t0 == t1) continue;
    a[3] += uint64_t(mS) * (t1 - t0);
    uint32_t mT = 0;
    for (uint32_t k = t0; k < t1; ++k) mT += T.ent[k].x == h;
    const uint64_t prod = uint64_t(mS) * mT;
    a[2] += prod;
    a[6] += prod;
    if (prod == 0) continue;
    if (prod <= kInline2) {
      // (two texts: with the empty LaneOut<false> in the counting kernel's text it compiled to
      // another register assignment than before)
      if constexpr (EMIT) {
        LaneOut<true> w(o, uint32_t(prod));  // the wave's active lanes reserve their slots together
        for (uint32_t ks = s0; ks < s1; ++ks) {
          const uint2 es = S.ent[ks];
          if (es.x != h) continue;
          for (uint32_t kt = t0; kt < t1; ++kt) {
            const uint2 et = T.ent[kt];
            if (et.x == h) {
              add_triple(a, pr, es.y, et.y, ck);
              w.put(pr, es.y, et.y);
            }
          }
        }
      } else {
        for (uint32_t ks = s0; ks < s1; ++ks) {
          const uint2 es = S.ent[ks];
          if (es.x != h) continue;
          for (uint32_t kt = t0; kt < t1; ++kt) {
            const uint2 et = T.ent[kt];
            if (et.x == h) add_triple(a, pr, es.y, et.y, ck);
          }
        }
      }
    } else {
      const uint64_t slot = atomicAdd(reinterpret_cast<unsigned long long*>(nheavy), 1ull);
      // (EMIT: the match counts travel with the item, k_chj_heavy places its triples by them)
      heavy[slot] = Heavy2{pr, h, EMIT ? mS : 0u, EMIT ? mT : 0u};
    }
  }
  block_flush<kF, 1>(a, res);
}

// Heavy chaining products: the block walks the S bucket; its threads stride over the T bucket.
// EMIT: the item's mS x mT triples take one slot range; the triple of the i-th matching S entry and
// the j-th matching T entry goes to slot i * mT + j of it. j comes from a workgroup prefix count over
// each chunk of kBlock T entries (ballot inside the wave, wave totals through LDS), so a wave's stores
// of one S entry are contiguous.
template <bool EMIT>
__global__ __launch_bounds__(kBlock) void k_chj_heavy(CTab S, CTab T, const Heavy2* __restrict__ heavy,
                                                      const uint64_t* __restrict__ nheavy, uint64_t* __restrict__ res,
                                                      bool ck, Out<EMIT> o) {
  uint64_t a[kF] = {0};
  const uint64_t nh = *nheavy;
  uint32_t it = 0;
  for (uint64_t q = blockIdx.x; q < nh; q += gridDim.x, ++it) {
    const Heavy2 hv = heavy[q];
    const uint32_t h = hv.ms;
    uint32_t s0, s1, t0, t1;
    S.range(h, &s0, &s1);
    T.range(h, &t0, &t1);
    if constexpr (EMIT) {
      constexpr int kWaves = kBlock / kWave;
      __shared__ uint32_t wcnt[2][kWaves];  // matching T entries per wave, chunks taking the rows in turn
      const uint32_t mT = hv.pad;
      const uint64_t prod = uint64_t(hv.mt) * mT;
      const Range<true> w(o, block_reserve<true>(o, prod, it), prod);
      const uint32_t lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
      uint32_t tb = 0, ch = 0;  // matching T entries before this chunk; chunk count
      for (uint32_t c = t0; c < t1; c += kBlock, ++ch) {  // (workgroup-uniform bounds: every thread meets the barrier)
        const uint32_t kt = c + threadIdx.x;
        uint2 et = make_uint2(0, 0);
        if (kt < t1) et = T.ent[kt];
        const bool m = kt < t1 && et.x == h;
        const uint64_t bal = __ballot(m);
        const uint32_t inw =
            __builtin_amdgcn_mbcnt_hi(uint32_t(bal >> 32), __builtin_amdgcn_mbcnt_lo(uint32_t(bal), 0u));
        if (lane == 0) wcnt[ch & 1][wid] = uint32_t(__popcll(bal));
        __syncthreads();
        uint32_t before = 0, all = 0;
#pragma unroll
        for (int x = 0; x < kWaves; ++x) {
          const uint32_t v = wcnt[ch & 1][x];
          all += v;
          before += uint32_t(x) < wid ? v : 0u;
        }
        const uint32_t j = tb + before + inw;
        tb += all;
        if (m) {
          uint64_t i = 0;
          for (uint32_t ks = s0; ks < s1; ++ks) {
            const uint2 es = S.ent[ks];
            if (es.x != h) continue;
            add_triple(a, hv.r, es.y, et.y, ck);
            w.put(i * mT + j, hv.r, es.y, et.y);
            ++i;
          }
        }
      }
    } else {
      for (uint32_t ks = s0; ks < s1; ++ks) {
        const uint2 es = S.ent[ks];
        if (es.x != h) continue;
        for (uint32_t kt = t0 + threadIdx.x; kt < t1; kt += kBlock) {
          const uint2 et = T.ent[kt];
          if (et.x == h) add_triple(a, hv.r, es.y, et.y, ck);
        }
      }
    }
  }
  block_flush<kF, 1>(a, res);
}

template <bool EMIT>
Out<EMIT> out_of(void* out, uint64_t out_cap, uint64_t* res) {
  if constexpr (EMIT)
    return Out<true>{static_cast<uint32_t*>(out), out_cap, reinterpret_cast<unsigned long long*>(res + kResCursor)};
  else
    return Out<false>{};
}

template <bool EMIT>
hipError_t probe2_on(hj3d_ctx* ctx, const hj3d_table* ts, const hj3d_table* tt, const hj3d_rel& r, uint32_t flags,
                     void* out, uint64_t out_cap, uint64_t* res, hipStream_t s) {
  const Out<EMIT> o = out_of<EMIT>(out, out_cap, res);
  const bool ck = flags & HJ3D_PROBE_CHECKSUM;  // triple hashes (sum_h, xor_h); row sums always
  // the result slot (the output cursor is one of its words) and the heavy-item counter start at zero:
  // one launch clears both (with the partitioner's own counters on the partitioned path)
  ZeroList z;
  z.add(res, kResFields);
  if (r.n == 0) return zero_words(z, s);
  hipError_t e = ctx->scratch[kScrC].ensure(r.n * sizeof(Heavy2) + 16);
  if (e != hipSuccess) return e;
  uint64_t* nheavy = ctx->scratch[kScrC].as<uint64_t>();
  Heavy2* heavy = reinterpret_cast<Heavy2*>(nheavy + 2);
  z.add(nheavy, 1);
  const RelView v = view_of(r);
  const unsigned g = grid_for(ctx, r.n, kBlock * kItems);
  if (ts->desc.kind == HJ3D_NESTED) {
    NTab S{ts->off.as<const uint32_t>(), ts->main.as<const uint4>(), ts->sub.as<const uint32_t>(), ts->fm,
           uint32_t(ts->desc.bucket_lo), ts->nb_local};
    NTab T{tt->off.as<const uint32_t>(), tt->main.as<const uint4>(), tt->sub.as<const uint32_t>(), tt->fm,
           uint32_t(tt->desc.bucket_lo), tt->nb_local};
    // partitioned when both tables share the bucket function (and their main counts are known)
    const bool same = ts->desc.num_buckets == tt->desc.num_buckets && ts->desc.bucket_lo == tt->desc.bucket_lo &&
                      ts->nb_local == tt->nb_local;
    e = hipErrorNotSupported;
    if (same && radix_nested_applicable(ctx, ts, r.n) && radix_nested_applicable(ctx, tt, r.n)) {
      const double fill = double(ts->n_mains + tt->n_mains) / double(ts->nb_local);
      ProbeParts pp;
      // no output: the regions' output slots are not needed
      e = radix_partition_probe(ctx, ts, r, uint32_t(kProbeWFrac * kProbeLdsWords / (2.0 + 4.0 * fill)), &pp, s, nullptr,
                                nullptr, false, &z);
      if (e == hipSuccess) {
        const uint32_t nblocks = pp.P * pp.splits;
        hipLaunchKernelGGL((k_ndu_seg<true, EMIT>), dim3(nblocks), dim3(kJBlock), 0, s, pp.region, pp.counts, pp.seg,
                           pp.G, pp.cap, S, T, pp.W, pp.P, pp.splits, pp.flat, heavy, nheavy, res, ck, o);
        hipLaunchKernelGGL((k_ndu_seg<false, EMIT>), dim3(nblocks), dim3(kJBlock), 0, s, pp.region, pp.counts, pp.seg,
                           pp.G, pp.cap, S, T, pp.W, pp.P, pp.splits, pp.flat, heavy, nheavy, res, ck, o);
        hipLaunchKernelGGL(k_ndu_ovf<EMIT>, dim3(ctx->num_cus), dim3(kBlock), 0, s, pp.ovf, pp.novf, S, T, heavy, nheavy,
                           res, ck, o);
      }
    }
    if (e == hipErrorNotSupported) {
      if ((e = zero_words(z, s)) != hipSuccess) return e;
      hipLaunchKernelGGL(k_ndu<EMIT>, dim3(g), dim3(kBlock), 0, s, v, S, T, heavy, nheavy, res, ck, o);
    } else if (e != hipSuccess) {
      return e;
    }
    hipLaunchKernelGGL(k_ndu_heavy<EMIT>, dim3(ctx->num_cus * 4), dim3(kBlock), 0, s, S, T, heavy, nheavy, res, ck, o);
  } else {
    if ((e = zero_words(z, s)) != hipSuccess) return e;
    CTab S{ts->off.as<const uint32_t>(), ts->ent.as<const uint2>(), ts->fm, uint32_t(ts->desc.bucket_lo),
           ts->nb_local};
    CTab T{tt->off.as<const uint32_t>(), tt->ent.as<const uint2>(), tt->fm, uint32_t(tt->desc.bucket_lo),
           tt->nb_local};
    hipLaunchKernelGGL(k_chj<EMIT>, dim3(g), dim3(kBlock), 0, s, v, S, T, heavy, nheavy, res, ck, o);
    hipLaunchKernelGGL(k_chj_heavy<EMIT>, dim3(ctx->num_cus * 4), dim3(kBlock), 0, s, S, T, heavy, nheavy, res, ck, o);
  }
  return hipGetLastError();
}

}  // namespace

hipError_t probe2(hj3d_ctx* ctx, const hj3d_table* ts, const hj3d_table* tt, const hj3d_rel& r, uint32_t flags,
                  void* out, uint64_t out_cap, uint64_t* res, hipStream_t s) {
  return (flags & HJ3D_PROBE_EMIT) ? probe2_on<true>(ctx, ts, tt, r, flags, out, out_cap, res, s)
                                   : probe2_on<false>(ctx, ts, tt, r, flags, out, out_cap, res, s);
}

}  // namespace hj3d
