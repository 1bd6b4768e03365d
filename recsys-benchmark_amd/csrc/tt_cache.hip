// tt_cache.hip — the LFU row cache of the TT-Rec table (`tt_emb`): frequency tracking and the hit / miss split
// (the lookup itself: the cached entry points of tt.hip).  Reference: src/models/embeddings/tt_embedding_ops.py:585-649 (buffers), :682-754 (call
// sequence update_cache -> preprocess_indices_sync -> tt_forward + cache_forward).  The FBTT kernels behind those
// calls are not in the reference tree; what follows is this build's own.
//
// hashtbl[S] (int64 ids, -1 empty) is an open-addressing table with linear probing:
//   start slot  id % S;  a probe stops at the id itself, at an empty slot, or after kProbeBound probes.
// The bound is the same for insert and find, so an id that was inserted is always found again, and an id that finds
// no slot within the bound stays untracked (the contraction serves it).  With S >= N (the default, S = N) this is
// direct addressing: slot == id, no collisions, and the state is reproducible bit for bit.
// Slots only ever go from empty to occupied (nothing deletes), so two lanes that insert the same new id walk the
// same probe sequence and end in the same slot: the loser of a compare-and-swap reads back the winner's id and stops
// there when it is its own.
//
// cache_freq[S] (int64) counts lookups per slot, cache_state[S] (int32) is the row of cache_weight that holds the
// slot's id, or -1.  k_probe_count does find-or-insert, the count and the state read for every lookup in ONE launch.
// A CTR field with a dominant value puts thousands of equal ids in one batch and a same-address atomic costs ~26 ns
// per adder, so the lanes of a wave that hold the same id elect one of them: it probes once and adds
// their number.  Integer atomics only.
#include "common.hpp"

namespace {
using namespace mi;

constexpr int kProbeBound = MI_TT_CACHE_PROBE_BOUND;

__device__ __forceinline__ long long load_slot(const long long *p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// slot of `id` in tbl[S], inserted where an empty slot comes first; -1 when the bound runs out
__device__ __forceinline__ long long probe(long long *tbl, long long S, long long id) {
  long long s = id % S;
  for (int t = 0; t < kProbeBound && t < S; ++t) {
    long long cur = load_slot(tbl + s);
    if (cur == id) return s;
    if (cur == -1) {
      unsigned long long seen = atomicCAS(reinterpret_cast<unsigned long long *>(tbl + s), (unsigned long long)-1LL,
                                          (unsigned long long)id);
      cur = (long long)seen;
      if (cur == -1 || cur == id) return s;        // won the slot, or lost it to a lane inserting the same id
    }
    s = s + 1 == S ? 0 : s + 1;
  }
  return -1;
}

__global__ __launch_bounds__(kBlock) void k_probe_count(const int64_t *__restrict__ idx, int64_t n, int64_t N,
                                                        long long *tbl, unsigned long long *freq,
                                                        const int32_t *__restrict__ state, long long S, int32_t C,
                                                        const int32_t *__restrict__ warm, int32_t *__restrict__ loc,
                                                        int *err) {
  const int lane = threadIdx.x & (kWave - 1);
  const bool warming = warm && *warm != 0;
  int bad = 0;
  // the trip count is the same for every lane of a wave: the election below uses wave-wide ballots
  for (int64_t i0 = (int64_t)blockIdx.x * blockDim.x; i0 < n; i0 += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = i0 + threadIdx.x;
    const bool active = i < n;
    long long id = active ? idx[i] : -1;
    const bool ok = active && (unsigned long long)id < (unsigned long long)N;
    bad |= active && !ok;
    // lanes holding the same id elect the lowest of them, which carries their number
    bool pending = ok;
    int leader = lane, count = 0;
    for (;;) {
      const unsigned long long todo = __ballot(pending);
      if (!todo) break;
      const int first = __ffsll(todo) - 1;
      const long long fid = __shfl(id, first);
      const bool same = pending && id == fid;
      const unsigned long long mates = __ballot(same);
      if (same) {
        leader = first;
        count = lane == first ? __popcll(mates) : 0;
        pending = false;
      }
    }
    long long slot = -1;
    if (ok && count > 0) {
      slot = probe(tbl, S, id);
      if (slot >= 0) atomicAdd(freq + slot, (unsigned long long)count);
    }
    slot = __shfl(slot, leader);
    if (active) {
      int32_t l = -1;
      if (ok && slot >= 0 && !warming) {
        l = state[slot];
        if ((uint32_t)l >= (uint32_t)C) l = -1;
      }
      loc[i] = l;
    }
  }
  if (bad && err) atomicOr(err, MI_IDX_OUT_OF_RANGE);
}

// re-insert the occupied (id, freq, state) triples of a table laid out by another rule
__global__ __launch_bounds__(kBlock) void k_rehash(const long long *__restrict__ ids, const long long *__restrict__ sfreq,
                                                   const int32_t *__restrict__ sstate, int64_t n, long long *tbl,
                                                   long long *freq, int32_t *state, long long S) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const long long id = ids[i];
    if (id < 0) continue;
    const long long slot = probe(tbl, S, id);
    if (slot < 0) continue;                       // no slot within the bound: the id is untracked from here on
    freq[slot] = sfreq[i];                        // an id occupies one source slot, so one lane writes a slot
    state[slot] = sstate[i];
  }
}

inline int grid_for(int64_t items) {
  int64_t g = (items + kBlock - 1) / kBlock;
  if (g < 1) g = 1;
  if (g > kMaxGrid) g = kMaxGrid;
  return (int)g;
}

}  // namespace

extern "C" {

int mi_tt_cache_probe_count(const int64_t *idx, int64_t n, int64_t N, int64_t *hashtbl, int64_t *cache_freq,
                            const int32_t *cache_state, int64_t hashtbl_size, int32_t cache_size,
                            const int32_t *warmup, int32_t *loc, int32_t *err, void *stream) {
  if (n < 0 || N < 0 || hashtbl_size < 1 || cache_size < 0) return MI_ERR_INVALID_ARG;
  if (n == 0) return MI_OK;
  if (!idx || !hashtbl || !cache_freq || !cache_state || !loc) return MI_ERR_INVALID_ARG;
  MI_LAUNCH("tt_cache_probe_count", k_probe_count, grid_for(n), kBlock, stream, idx, n, N,
            reinterpret_cast<long long *>(hashtbl), reinterpret_cast<unsigned long long *>(cache_freq), cache_state,
            (long long)hashtbl_size, cache_size, warmup, loc, err);
  return launch_status();
}

int mi_tt_cache_rehash(const int64_t *src_ids, const int64_t *src_freq, const int32_t *src_state, int64_t n_src,
                       int64_t *hashtbl, int64_t *cache_freq, int32_t *cache_state, int64_t hashtbl_size,
                       void *stream) {
  if (n_src < 0 || hashtbl_size < 1) return MI_ERR_INVALID_ARG;
  if (n_src == 0) return MI_OK;
  if (!src_ids || !src_freq || !src_state || !hashtbl || !cache_freq || !cache_state) return MI_ERR_INVALID_ARG;
  if (src_ids == hashtbl || src_freq == cache_freq || src_state == cache_state) return MI_ERR_INVALID_ARG;
  MI_LAUNCH("tt_cache_rehash", k_rehash, grid_for(n_src), kBlock, stream, reinterpret_cast<const long long *>(src_ids),
            reinterpret_cast<const long long *>(src_freq), src_state, n_src, reinterpret_cast<long long *>(hashtbl),
            reinterpret_cast<long long *>(cache_freq), cache_state, (long long)hashtbl_size);
  return launch_status();
}

}  // extern "C"
