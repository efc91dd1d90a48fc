// arena_rows.h — leaf rows: batch dedup, the evaluation cache, the peer push, k_scan_need, k_encode.
// Included by spmcts.hip after arena_select.h: needs View and the helpers of arena_select.h.
// ----------------------------------------------------------------------------
// kernel: compaction of pending leaves into rows (tree order => deterministic)
// ----------------------------------------------------------------------------
// Two segments: leaves of network-0 trees in rows [0, n0), of network-1 trees in rows
// [seg1, seg1 + n1) (single-network arenas: seg1 = T, n1 = 0).
// count_out (optional): [0] = n0 + n1, [1] = n0, [2] = n1.
// ----------------------------------------------------------------------------
// batch leaf dedup (K > 1): the network input of a pending leaf is its (own, opp) stone planes from
// the mover's view (k_encode), so leaves with equal (own, opp) of the same network get one row and
// one evaluation; the trunk and heads are deterministic and batch-independent, so every leaf still
// receives exactly the outputs its own row would have produced.  Owner of a key = its lowest slot
// (deterministic); the table is cleared by generation stamps instead of a memset per step.
// ----------------------------------------------------------------------------
// SYM (spmcts_set_symmetry): the key is the canonical pair (board.h, canonical_pair), so a position and its mirror
// image share a row, a peer row and a cache record; every kernel that takes a key is instantiated for both modes,
// and the SYM = false ones are the kernels of an arena without the mode (View has no field for it).
// k_dedup_insert recomputes the key of the slot it collides with on every probe: with SYM that is the mirror's
// register arithmetic behind the three loads the key already costs, and no per-slot state to keep current.
template <class G, bool SYM = false>
__device__ __forceinline__ void leaf_key(const View &v, int t, uint64_t &own, uint64_t &opp) {
  const int mover = v.lmover[t];
  own = mover > 0 ? v.lpos[t] : v.lneg[t];
  opp = mover > 0 ? v.lneg[t] : v.lpos[t];
  if constexpr (SYM) canonical_pair<G>(own, opp);
  if (v.tnet[t / v.K]) own |= 1ull << 63;  // rows of the two networks never merge (cell bits < 63)
}

__device__ __forceinline__ uint32_t leaf_hash(uint64_t a, uint64_t b) {
  uint64_t x = a ^ (b * 0x9E3779B97F4A7C15ull);
  x ^= x >> 33;
  x *= 0xff51afd7ed558ccdull;
  x ^= x >> 33;
  x *= 0xc4ceb9fe1a85ec53ull;
  x ^= x >> 33;
  return (uint32_t)x;
}

template <class G, bool SYM = false>
__global__ __launch_bounds__(256) void k_dedup_insert(View v) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= v.dn * v.K) return;
  const int t = dom_slot(v, c);
  if (t < 0 || v.need[t] != NEED_ROW) return;  // (a NEED_STASH slot is evaluated already: no row, here and below)
  uint64_t own, opp;
  leaf_key<G, SYM>(v, t, own, opp);
  const unsigned long long mine = ((unsigned long long)v.dgen << 32) | (uint32_t)t;
  unsigned long long *tab = (unsigned long long *)v.dtab;
  uint32_t h = leaf_hash(own, opp) & (uint32_t)v.dmask;
  for (int probe = 0; probe <= v.dmask; ++probe) {
    // claim the entry if it holds an older generation; a failed CAS returns the current value, which
    // during this kernel can only have become this generation's (at most two rounds)
    unsigned long long w = tab[h];
    while ((uint32_t)(w >> 32) != v.dgen) {
      const unsigned long long old = atomicCAS(tab + h, w, mine);
      if (old == w) {
        v.dent[t] = (int)h;
        return;
      }
      w = old;
    }
    uint64_t so, sp;
    leaf_key<G, SYM>(v, (int)(uint32_t)w, so, sp);
    if (so == own && sp == opp) {
      atomicMin(tab + h, mine);  // the lowest slot of the key owns the row
      v.dent[t] = (int)h;
      return;
    }
    h = (h + 1) & (uint32_t)v.dmask;
  }
  set_err(v, SPMCTS_ERR_STATE);  // unreachable: the table has >= 2 NS entries
}

// owner flags, one independent load pair per slot, and the row flag of each compact index of the launch
// domain (crow: the scan below then reads consecutive words instead of a dependent dent -> dtab chain per
// slot in its serial chunk loop; without dedup every pending slot owns its row); a leader lane also
// keeps each owner's key for its followers' lookups this step (okey: nothing else writes it until its
// next step's k_dedup_owner, which runs after every follower's lookup of this step)
// Evaluation cache (spmcts_set_eval_cache): linear probing over at most CACHE_PROBES entries from the key's
// hash.  An entry's tag is (generation << 32 | state): 0 = never used, CACHE_READY = key and outputs published,
// CACHE_BUSY = being written.  A lookup sees READY entries whose generation is within the window of its own
// (0 <= cgen - gen < cwin); an insert may take an entry that was never used or whose READY generation is more
// than cwin behind its own (one generation of slack: the two lanes of a shared table are at most one ply apart,
// so no entry a lane can still see, or renew, is taken by the other).  Tags never return to 0, so every entry
// before a live key's entry in its probe chain has been in use since the key went in, and a lookup may stop at
// the first never-used entry.  Publication: CAS to BUSY, key and outputs stored, then the READY tag stored with
// release semantics (agent scope); a lookup confirms a candidate by acquire re-reads (cache_find), so a READY key
// is never read torn (a lane sharing its leader's table reads it while the leader's expand inserts on another
// stream).
constexpr int CACHE_PROBES = 32;
constexpr unsigned long long CACHE_READY = 1ull, CACHE_BUSY = 2ull;

constexpr int CACHE_REC = 8;  // u64 words per record (64 bytes): tag, own, opp, (A + 1) f32 (A <= 9)
static_assert(24 + 4 * (C4::A + 1) <= 8 * CACHE_REC && 24 + 4 * (TTT::A + 1) <= 8 * CACHE_REC &&
                  24 + 4 * (C4_6x5::A + 1) <= 8 * CACHE_REC && 24 + 4 * (C4_8x7::A + 1) <= 8 * CACHE_REC,
              "cache record");

__device__ __forceinline__ unsigned long long *cache_rec(const View &v, uint32_t h) {
  return (unsigned long long *)v.crec + (size_t)h * CACHE_REC;
}
__device__ __forceinline__ float *cache_out(const View &v, uint32_t h) {
  return (float *)(cache_rec(v, h) + 3);
}

__device__ __forceinline__ bool cache_live_tag(const View &v, unsigned long long tag) {
  const int d = (int)(v.cgen - (uint32_t)(tag >> 32));
  return (tag & 0xffffffffull) == CACHE_READY && d >= 0 && d < v.cwin;
}

__device__ __forceinline__ bool cache_free_tag(const View &v, unsigned long long tag) {
  const int d = (int)(v.cgen - (uint32_t)(tag >> 32));
  return tag == 0 || ((tag & 0xffffffffull) == CACHE_READY && d > v.cwin);
}

// The probe loop reads records with plain loads (a stale line only makes a miss or an early stop: the position
// is then evaluated); a candidate is confirmed after an acquire fence by atomic re-reads of its tag and key, so a
// hit is a READY record whose key and outputs were published before the tag.
__device__ __forceinline__ int cache_find(const View &v, uint64_t own, uint64_t opp) {
  uint32_t h = leaf_hash(own, opp) & (uint32_t)v.cmask;
  for (int p = 0; p < CACHE_PROBES; ++p) {
    const unsigned long long *r = cache_rec(v, h);
    const unsigned long long tag = r[0];
    if (tag == 0) return -1;
    if (cache_live_tag(v, tag) && r[1] == own && r[2] == opp) {
      __atomic_thread_fence(__ATOMIC_ACQUIRE);
      unsigned long long *rw = cache_rec(v, h);
      const unsigned long long t2 = __hip_atomic_load(rw, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
      const unsigned long long o2 = __hip_atomic_load(rw + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const unsigned long long q2 = __hip_atomic_load(rw + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      return cache_live_tag(v, t2) && o2 == own && q2 == opp ? (int)h : -1;
    }
    h = (h + 1) & (uint32_t)v.cmask;
  }
  return -1;
}

// an owner slot's key in the cache: down 3, the entry in xc, its generation renewed (kept while in use)
template <class G, bool SYM = false>
__device__ __forceinline__ bool cache_hit(const View &v, int t) {
  uint64_t own, opp;
  leaf_key<G, SYM>(v, t, own, opp);
  const int e = cache_find(v, own, opp);
  if (e < 0) return false;
  __hip_atomic_store(cache_rec(v, e), ((unsigned long long)v.cgen << 32) | CACHE_READY, __ATOMIC_RELAXED,
                     __HIP_MEMORY_SCOPE_AGENT);
  v.xc[t] = e;
  return true;
}

template <class G, bool SYM = false>
__global__ __launch_bounds__(256) void k_dedup_owner(View v) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= v.dn * v.K) return;
  const int t = dom_slot(v, c);
  int d = 0;
  if (t >= 0 && !v.dedup) {
    d = v.need[t] == NEED_ROW;  // no dedup: every leaf that waits for the network owns its row
  } else if (t >= 0) {
    const bool own = v.need[t] == NEED_ROW && (int)(uint32_t)v.dtab[v.dent[t]] == t;
    d = own ? (v.cwin && cache_hit<G, SYM>(v, t) ? 3 : 1) : 0;
    v.down[t] = (uint8_t)d;
    if (own && v.lead) {
      uint64_t a, b;
      leaf_key<G, SYM>(v, t, a, b);
      v.okey[2 * (size_t)t] = a;
      v.okey[2 * (size_t)t + 1] = b;
    }
  }
  v.crow[c] = d ? t * 4 + d : 0;
}

// Follower lane (spmcts_set_leaf_peer), a simulation step: owner flags as k_dedup_owner, and each owner
// slot's key looked up in the leader lane's table of the same step (generation pgen, probed as the
// leader's k_dedup_insert placed it: a key present this generation sits before the first entry of an
// older one).  A hit takes the leader's row: down 2, xpeer = the leader's owner slot.  Outputs are pure
// functions of the leaf planes (the fused trunk is batch-independent), so the leaf still gets exactly
// the outputs its own row would have produced.
template <class G, bool SYM = false>
__global__ __launch_bounds__(256) void k_dedup_owner_peer(View v, const uint64_t *ptab, const uint64_t *pkey,
                                                          const uint8_t *pdown, int pmask, uint32_t pgen) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= v.dn * v.K) return;
  const int t = dom_slot(v, c);
  if (t < 0) {
    v.crow[c] = 0;
    return;
  }
  int d = 0, xp = -1;
  if (v.need[t] == NEED_ROW && (int)(uint32_t)v.dtab[v.dent[t]] == t) {
    d = 1;
    if (v.cwin && cache_hit<G, SYM>(v, t)) {  // the follower's own cache first: no wait on the leader's outputs
      v.down[t] = 3;
      v.xpeer[t] = -1;
      v.crow[c] = t * 4 + 3;
      return;
    }
    uint64_t own, opp;
    leaf_key<G, SYM>(v, t, own, opp);
    uint32_t h = leaf_hash(own, opp) & (uint32_t)pmask;
    for (int probe = 0; probe <= pmask; ++probe) {
      const unsigned long long w = ptab[h];
      if ((uint32_t)(w >> 32) != pgen) break;  // not in the leader's batch
      const int s = (int)(uint32_t)w;
      if (pkey[2 * (size_t)s] == own && pkey[2 * (size_t)s + 1] == opp) {
        if (pdown[s] == 1) {  // a row the leader's network evaluates (not one its cache fills at its expand)
          d = 2;
          xp = s;
        }
        break;
      }
      h = (h + 1) & (uint32_t)pmask;
    }
  }
  v.down[t] = (uint8_t)d;
  v.xpeer[t] = xp;
  v.crow[c] = d ? t * 4 + d : 0;
}

// the leader's outputs of this step into the follower's rows of the slots it serves (down 2), on the
// leader's stream after its heads (spmcts_peer_push): probs [row][A] f32, values [row] f32
__global__ __launch_bounds__(256) void k_peer_push(View v, const int32_t *psrow, const float *pprobs,
                                                   const float *pvalues, float *probs, float *values) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= v.dn * v.K) return;
  const int t = dom_slot(v, c);
  if (t < 0 || v.down[t] != 2) return;
  const int r1 = v.srow[t], r0 = psrow[v.xpeer[t]];
  for (int a = 0; a < v.A; ++a) probs[(size_t)r1 * v.A + a] = pprobs[(size_t)r0 * v.A + a];
  values[r1] = pvalues[r0];
}

// Evaluation cache at the expand of a step whose rows consulted it (single-network arenas): a cache-served
// owner slot (down 3) gets its entry's outputs in its row; a slot whose row holds network outputs (down 1:
// its own network's, down 2: the leader's, pushed before this -- unless the table is the leader's own, which
// the leader fills) puts them in the cache under the current generation (nothing is cached when no entry
// within CACHE_PROBES is free).  Duplicates (down 0) read their owner's row.
template <class G, bool SYM = false>
__global__ __launch_bounds__(256) void k_cache_io(View v, float *probs0, float *values0, float *probs1,
                                                  float *values1) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= v.dn * v.K) return;
  const int t = dom_slot(v, c);
  if (t < 0 || v.need[t] != NEED_ROW) return;
  const int d = v.down[t];
  if (d == 0) return;
  const int A = v.A;
  // network-1 rows (two-network arenas) live in their own output buffers, indexed by row - seg1
  const int row = v.srow[t];
  const bool n1 = row >= v.seg1;
  const int r = n1 ? row - v.seg1 : row;
  float *values = n1 ? values1 : values0;
  float *pr = (n1 ? probs1 : probs0) + (size_t)r * A;
  if (d == 3) {
    const float *c = cache_out(v, v.xc[t]);
    for (int a = 0; a < A; ++a) pr[a] = c[a];
    values[r] = c[A];
    return;
  }
  if (d == 2 && v.cshared) return;
  uint64_t own, opp;
  leaf_key<G, SYM>(v, t, own, opp);
  uint32_t h = leaf_hash(own, opp) & (uint32_t)v.cmask;
  const unsigned long long gen = (unsigned long long)v.cgen << 32;
  for (int p = 0; p < CACHE_PROBES; ++p) {
    unsigned long long *rec = cache_rec(v, h);
    unsigned long long w = __hip_atomic_load(rec, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    while (cache_free_tag(v, w)) {  // never used, or behind the window (+1): free to take
      const unsigned long long old = atomicCAS(rec, w, gen | CACHE_BUSY);
      if (old == w) {
        rec[1] = own;
        rec[2] = opp;
        float *c = cache_out(v, h);
        for (int a = 0; a < A; ++a) c[a] = pr[a];
        c[A] = values[r];
        __hip_atomic_store(rec, gen | CACHE_READY, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
        return;
      }
      w = old;  // another insert took it first: probe on
    }
    h = (h + 1) & (uint32_t)v.cmask;
  }
}

// duplicates read their owner's row
__global__ __launch_bounds__(256) void k_dedup_alias(View v) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= v.dn * v.K) return;
  const int t = dom_slot(v, c);
  if (t < 0 || v.need[t] != NEED_ROW) return;
  const int s = (int)(uint32_t)v.dtab[v.dent[t]];
  if (s != t) v.srow[t] = v.srow[s];
}

// 512 threads = two waves per SIMD: the kernel runs while the other lane's trunk holds every CU, in the
// registers a trunk wave leaves free on its SIMD (512 - 424 = 88 per lane beside the C = 128 trunk; a
// 1,024-thread block needs 4 x 24 there and waited for a trunk workgroup to retire: 37 -> 90 us average
// in the bench trace, profiles/r04_bench_prof/; 256 threads: 64 us, two rounds of flag loads per pass)
constexpr int SCAN_THREADS = 512;
constexpr int SCAN_WAVES = SCAN_THREADS / 64;
constexpr int SCAN_BATCH = 20;  // words of crow past its NS entries (a batch is loaded whole, then masked)

// One thread's chunk [lo, hi) of the step's row flags (View::crow, the domain's compact order): f(slot, d, n1)
// for each slot with a row, in order.  d: 1 = a row its network evaluates, 2 / 3 = a served row (leader /
// cache); n1: a network-1 tree's slot.  SCAN_BATCH flags at a time, one round of independent loads of
// consecutive words (and one of the trees' networks in a two-network arena): the bench's lanes have 16 or 17
// slots per thread, one batch.
template <class F>
__device__ __forceinline__ void scan_chunk(const View &v, int lo, int hi, F &&f) {
  for (int base = lo; base < hi; base += SCAN_BATCH) {
    int e[SCAN_BATCH];
    uint32_t n1 = 0;
#pragma unroll
    for (int u = 0; u < SCAN_BATCH; ++u) e[u] = v.crow[base + u];
#pragma unroll
    for (int u = 0; u < SCAN_BATCH; ++u)
      if (base + u >= hi) e[u] = 0;
    if (v.seg1 < v.NS) {  // two-network arena (single-network: no tnet loads)
#pragma unroll
      for (int u = 0; u < SCAN_BATCH; ++u) n1 |= (v.tnet[(e[u] >> 2) / v.K] ? 1u : 0u) << u;
    }
#pragma unroll
    for (int u = 0; u < SCAN_BATCH; ++u)
      if (e[u]) f(e[u] >> 2, e[u] & 3, ((n1 >> u) & 1u) != 0);
  }
}

__global__ __launch_bounds__(SCAN_THREADS) void k_scan_need(View v, int32_t *count_out) {
  // wave totals of the two segments' owner counts (a two-level scan: 6 shuffle steps within each wave,
  // 3 over the 8 wave totals, 2 barriers; the round-3 1,024-entry Hillis-Steele scan took 20 barriers
  // and 8 KB of LDS)
  __shared__ int32_t s_w0[SCAN_WAVES], s_w1[SCAN_WAVES], s_w2[SCAN_WAVES], s_w4[SCAN_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // the domain's pending slots in compact order (list entry, then in-flight index): slot order, as the list
  // ascends; each thread a contiguous chunk of them
  const int T = v.dn * v.K;
  const int chunk = (T + SCAN_THREADS - 1) / SCAN_THREADS;
  const int lo = min(T, tid * chunk), hi = min(T, lo + chunk);
  // c0 / c1: network-0 / network-1 rows the networks evaluate; c2 / c4: served rows (leader- or cache-served) of
  // network 0 / 1, numbered after the evaluated rows of their segment; c3: cache-served rows (a counter)
  int c0 = 0, c1 = 0, c2 = 0, c3 = 0, c4 = 0;
  scan_chunk(v, lo, hi, [&](int, int d, bool n1) {
    c0 += d == 1 && !n1;
    c1 += d == 1 && n1;
    c2 += d >= 2 && !n1;
    c4 += d >= 2 && n1;
    c3 += d == 3;
  });
  // inclusive scans of (c0, c1, c2, c4) in thread order: within the wave, then over the wave totals
  int i0 = c0, i1 = c1, i2 = c2, i4 = c4;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int a0 = __shfl_up(i0, off, 64), a1 = __shfl_up(i1, off, 64), a2 = __shfl_up(i2, off, 64);
    const int a4 = __shfl_up(i4, off, 64);
    if (lane >= off) {
      i0 += a0;
      i1 += a1;
      i2 += a2;
      i4 += a4;
    }
  }
  if (lane == 63) {
    s_w0[wave] = i0;
    s_w1[wave] = i1;
    s_w2[wave] = i2;
    s_w4[wave] = i4;
  }
  __syncthreads();
  if (wave == 0) {
    int w0 = lane < SCAN_WAVES ? s_w0[lane] : 0, w1 = lane < SCAN_WAVES ? s_w1[lane] : 0;
    int w2 = lane < SCAN_WAVES ? s_w2[lane] : 0, w4 = lane < SCAN_WAVES ? s_w4[lane] : 0;
#pragma unroll
    for (int off = 1; off < SCAN_WAVES; off <<= 1) {
      const int a0 = __shfl_up(w0, off, 64), a1 = __shfl_up(w1, off, 64), a2 = __shfl_up(w2, off, 64);
      const int a4 = __shfl_up(w4, off, 64);
      if (lane >= off) {
        w0 += a0;
        w1 += a1;
        w2 += a2;
        w4 += a4;
      }
    }
    if (lane < SCAN_WAVES) {
      s_w0[lane] = w0;
      s_w1[lane] = w1;
      s_w2[lane] = w2;
      s_w4[lane] = w4;
    }
  }
  __syncthreads();
  i0 += wave ? s_w0[wave - 1] : 0;
  i1 += wave ? s_w1[wave - 1] : 0;
  i2 += wave ? s_w2[wave - 1] : 0;
  i4 += wave ? s_w4[wave - 1] : 0;
  // served rows follow all evaluated rows of their network's segment
  int r0 = i0 - c0, r1 = v.seg1 + i1 - c1;
  int r2 = s_w0[SCAN_WAVES - 1] + i2 - c2, r4 = v.seg1 + s_w1[SCAN_WAVES - 1] + i4 - c4;
  scan_chunk(v, lo, hi, [&](int t, int d, bool n1) {
    if (d == 1) {
      const int r = n1 ? r1++ : r0++;
      v.row_tree[r] = t;
      if (v.K > 1) v.srow[t] = r;
    } else {
      v.srow[t] = n1 ? r4++ : r2++;
    }
  });
  if (v.cwin) {  // cache-served rows (counters.cache_rows)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) c3 += __shfl_xor(c3, off, 64);
    if (lane == 0 && c3) atomicAdd((unsigned long long *)&v.gcnt[11], (unsigned long long)c3);
  }
  if (tid == SCAN_THREADS - 1) {  // the last thread's inclusive prefix is each segment's total
    v.row_count[0] = i0;
    v.row_count[1] = i1;
    v.gcnt[10] += i0 + i1;  // network rows emitted (counters.nn_rows)
    if (count_out) {
      count_out[0] = i0 + i1;
      count_out[1] = i0;
      count_out[2] = i1;
    }
  }
}

__device__ __forceinline__ bool row_live(const View &v, int row) {
  return row < v.seg1 ? row < v.row_count[0] : row - v.seg1 < v.row_count[1];
}

// ----------------------------------------------------------------------------
// kernel: leaf encoding (preprocess, games/general/modules.py:115-125; input = state*mover)
// ----------------------------------------------------------------------------
template <class G, bool SYM = false>
__global__ void k_encode(View v, void *out) {
  const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int cell = (int)(gid % G::CELLS);
  // the i-th live row: network 0's n0 rows from row 0, then network 1's n1 from row seg1 (n0 + n1 <= dn * K:
  // a pending slot of the domain owns at most one row)
  const int i = (int)(gid / G::CELLS), n0 = v.row_count[0];
  if (i >= v.dn * v.K || i - n0 >= v.row_count[1]) return;
  const int row = i < n0 ? i : v.seg1 + i - n0;
  const int t = v.row_tree[row];
  const int x = cell / G::H, y = cell % G::H;
  const uint64_t bit = 1ull << cell_bit<G>(x, y);
  const int mover = v.lmover[t];
  uint64_t own = mover > 0 ? v.lpos[t] : v.lneg[t];
  uint64_t opp = mover > 0 ? v.lneg[t] : v.lpos[t];
  if constexpr (SYM) canonical_pair<G>(own, opp);  // the row in canonical orientation: cell (x, y) of the mirror image
  const int c_own = (own & bit) ? 1 : 0, c_opp = (opp & bit) ? 1 : 0;
  const int c_emp = 1 - c_own - c_opp;
  if (v.leaf_format == SPMCTS_LEAF_BOARD_I64) {
    ((int64_t *)out)[(size_t)row * G::CELLS + cell] = (int64_t)(c_own - c_opp);
    return;
  }
  size_t i0, i1, i2;
  if (v.leaf_layout == SPMCTS_NHWC) {
    const size_t base = ((size_t)row * G::CELLS + cell) * 3;
    i0 = base;
    i1 = base + 1;
    i2 = base + 2;
  } else {
    const size_t base = (size_t)row * 3 * G::CELLS + cell;
    i0 = base;
    i1 = base + G::CELLS;
    i2 = base + 2 * G::CELLS;
  }
  if (v.leaf_format == SPMCTS_LEAF_F32) {
    float *o = (float *)out;
    o[i0] = (float)c_emp;
    o[i1] = (float)c_own;
    o[i2] = (float)c_opp;
  } else {
    const uint16_t one = v.leaf_format == SPMCTS_LEAF_F16 ? 0x3C00 : 0x3F80;
    uint16_t *o = (uint16_t *)out;
    o[i0] = c_emp ? one : 0;
    o[i1] = c_own ? one : 0;
    o[i2] = c_opp ? one : 0;
  }
}
