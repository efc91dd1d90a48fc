// arena_rng.h — the per-tree RNG: Philox (rocRAND) or the parity tape.
// Included by spmcts.hip after arena_view.h: needs View and philox.h.
// ----------------------------------------------------------------------------
// RNG: Philox (rocRAND) or parity tape
// ----------------------------------------------------------------------------
struct TreeRng {
  PhiloxFields f;  // Philox mode: counter, key, substate (f.result is not carried; rng_store rebuilds it)
  int64_t cur, end;
};

__device__ __forceinline__ void rng_load(const View &v, int tree, TreeRng &r) {
  if (v.rng_mode == SPMCTS_RNG_TAPE) {
    r.cur = v.tape_cur[tree];
    r.end = v.tape_end[tree];
  } else {
    // memcpy: the rocRAND object read as its leading fields, without a type-punned access
    __builtin_memcpy(&r.f, (const void *)(v.rng + tree), sizeof(PhiloxFields));
  }
}

__device__ __forceinline__ void rng_store(const View &v, int tree, const TreeRng &r) {
  if (v.rng_mode == SPMCTS_RNG_TAPE) {
    v.tape_cur[tree] = r.cur;
  } else {
    // the state's leading fields, with rocRAND's output block rebuilt (philox.h); its Box-Muller
    // cache (the trailing fields, used only by the Dirichlet draws) is left as it was
    PhiloxFields f = r.f;
    philox_sync(f);
    __builtin_memcpy((void *)(v.rng + tree), &f, sizeof(PhiloxFields));
  }
}

// One double in [0, 1) for lane `j` of a k-wide vector draw (all lanes call it with the
// same state; the shared state then advances by k via rng_advance).
__device__ __forceinline__ double rng_lane(const View &v, const TreeRng &r, int j, bool *tape_err) {
  if (v.rng_mode == SPMCTS_RNG_TAPE) {
    const int64_t i = r.cur + j;
    if (i >= r.end) {
      *tape_err = true;
      return 0.0;
    }
    return v.tape[i];
  }
  // = skipahead(2j) + rocrand_uniform_double, without the run-time index into the output block
  return 1.0 - philox_uniform_at(r.f, 2ull * (unsigned long long)j);  // rocRAND gives (0, 1]
}

__device__ __forceinline__ void rng_advance(const View &v, TreeRng &r, int k) {
  if (v.rng_mode == SPMCTS_RNG_TAPE)
    r.cur += k;
  else
    philox_skip(r.f, 2ull * (unsigned long long)k);  // skipahead(2k) minus its output-block refresh
}

// Child jitter of a P-lane tree group, lane j < A using its draw (= rng_lane(j)); every lane of the
// group must call it.  Tape mode reads lane j's tape entry; Philox mode computes each output block
// once per group and shares it through shuffles (philox.h philox_uniform_group).
template <class G>
__device__ __forceinline__ double rng_group(const View &v, const TreeRng &r, int lane, int gbase, bool *tape_err) {
  if (v.rng_mode == SPMCTS_RNG_TAPE) return lane < G::A ? rng_lane(v, r, lane, tape_err) : 0.0;
  return 1.0 - philox_uniform_group<G::APAD>(r.f, lane, gbase);
}

// sequential scalar draw (single thread)
__device__ __forceinline__ double rng_next(const View &v, TreeRng &r, bool *tape_err) {
  double u = rng_lane(v, r, 0, tape_err);
  rng_advance(v, r, 1);
  return u;
}

// Gamma(alpha, 1): alpha == 1 -> Exp(1) = -log U; otherwise Marsaglia-Tsang.
__device__ double gamma_draw(Philox *s, double alpha) {
  if (alpha == 1.0) return -log(rocrand_uniform_double(s));
  double boost = 1.0;
  if (alpha < 1.0) {
    boost = pow(rocrand_uniform_double(s), 1.0 / alpha);
    alpha += 1.0;
  }
  const double d = alpha - 1.0 / 3.0, c = 1.0 / sqrt(9.0 * d);
  for (int it = 0; it < 256; ++it) {
    const double xn = rocrand_normal_double(s);
    double t = 1.0 + c * xn;
    if (t <= 0.0) continue;
    t = t * t * t;
    const double u = rocrand_uniform_double(s);
    if (log(u) < 0.5 * xn * xn + d - d * t + d * log(t)) return d * t * boost;
  }
  return d * boost;
}
