// rd_feed_aug.hip -- the batch feed (rd_feed.hip) with train-time input augmentation in the same launch: time-step drop with
// compaction, sensor drop, observation drop and value jitter, applied while the batch is formed (DESIGN §3e').
//
// One launch, the copy structure of k_batch_gather / k_feed_gather (rd_feed.hip: 16 batch rows x 16 lanes per copy workgroup, one
// wavefront per sample for lengths / label / statics), no dependence between workgroups, no atomics but the integer `bad` counter,
// the batch written once.  Every decision is a pure function of a batch key and SOURCE coordinates (rd_rng.h uniform4, keep iff
// u >= p), so a replay, a warm-up pass whose cursor is put back, and the host restatement (tests/feed_aug_ref.py) agree bit for bit.
//   key = seed + draw,  draw = epoch * capacity + cursor (feed form) or the caller's (explicit-index form)
//   cell = {u64 seed, u64 epoch, f32 p_time, f32 p_sensor, f32 p_obs, f32 noise_c}, read when the kernel RUNS
// W = 2F: columns [0, F) are values, [F, 2F) the observed-indicators.  b: slot in the batch, t: row of the SOURCE sample.
//   1. time-step drop (SITE_FEED_TIME, element b*T + t): candidates are the rows t < L, L = #{t : time[t] > 0}; a sample whose
//      candidates would all go keeps all of them.  Output rows: the kept candidates in order, then the source rows [L, T)
//      unchanged, then rows of +0.0 -- src and times alike; lengths is the count of written times > 0.
//   2. sensor drop (SITE_FEED_SENSOR, element b*F + f): value and indicator +0.0 in every row.
//   3. observation drop (SITE_FEED_OBS, element (t*B + b)*F + f): value and indicator +0.0.
//   4. jitter (SITE_FEED_NOISE, the whole quad (t*B + b)*F + f) where the indicator is still non-zero:
//      v' = fmaf(((u.x + u.y) + (u.z + u.w)) - 2, noise_c, v) -- Irwin-Hall(4), no transcendental, one rounding.
// A rate of exactly 0 makes no generator call for its transform; all four at 0 write k_batch_gather's bytes.
//
// The compaction needs, per (sample, output row), the source row.  A copy workgroup's wave w holds the copy lanes of exactly the
// batch slots 4w .. 4w+3, so each wave works out its own four look-ups and nothing crosses waves (no LDS, no barrier): per sample
// the time column is counted by wave-wide ballots in passes of 64 rows, then the keep bits of the candidates are drawn in passes of
// 64 with a running base until the pass that holds the wanted rank.  Every workgroup that needs a sample's keep bits redraws them.
#include "rd_common.h"
#include "rd_rng.h"

namespace rd {
namespace {

constexpr int FA_RPB = 16;        // batch rows per copy workgroup (rd_feed.hip FD_RPB)

struct AugArgs {
  const float *P_all, *time_all, *static_all;
  const int64_t *y_all, *idx;
  float *src, *times, *static_out;
  int64_t *y_out, *lengths;
  int32_t* bad;
  const uint64_t* aug;            // the 32-byte cell
  long N;
  int T, B, W, F, ds, ncopy, nbg, vec;
};

struct AugRates { uint64_t key; float p_time, p_sensor, p_obs, noise_c; };

// rd_feed.hip checked_index: an out-of-range index is counted and clamped
__device__ __forceinline__ long checked_index(const AugArgs& a, int b, bool count) {
  long n = a.idx[b];
  if (n < 0 || n >= a.N) {
    if (count && a.bad) atomicAdd(a.bad, 1);
    n = n < 0 ? 0 : a.N - 1;
  }
  return n;
}

// rd_feed.hip feed_cursor: the plan row actually read always lies inside the plan
__device__ __forceinline__ long feed_cursor(const int64_t* cell, long capacity, bool& ok) {
  const long k = (long)load_uniform_u64(reinterpret_cast<const uint64_t*>(cell));
  long nb = (long)load_uniform_u64(reinterpret_cast<const uint64_t*>(cell + 1));
  nb = nb < capacity ? nb : capacity;
  ok = k >= 0 && k < nb;
  return ok ? k : (nb > 0 ? nb - 1 : 0);
}

__device__ __forceinline__ float comp4(const float4& u, int j) { return j == 0 ? u.x : (j == 1 ? u.y : (j == 2 ? u.z : u.w)); }

__device__ __forceinline__ float uniform1(uint64_t key, uint32_t site, uint64_t idx) {
  return comp4(uniform4(key, site, idx >> 2), (int)(idx & 3));
}

// the uniforms of elements idx and idx + 1: one generator call unless the pair straddles two quads
__device__ __forceinline__ void uniform2(uint64_t key, uint32_t site, uint64_t idx, float& u0, float& u1) {
  float4 q = uniform4(key, site, idx >> 2);
  u0 = comp4(q, (int)(idx & 3));
  if ((idx & 3) == 3) q = uniform4(key, site, (idx + 1) >> 2);
  u1 = comp4(q, (int)((idx + 1) & 3));
}

__device__ __forceinline__ float jitter(const AugRates& r, uint64_t quad, float v) {
  const float4 u = uniform4(r.key, SITE_FEED_NOISE, quad);
  const float s = (u.x + u.y) + (u.z + u.w);                  // multiples of 2^-16 below 4: exact
  return __fmaf_rn(s - 2.f, r.noise_c, v);
}

// L = #{t : time[t] > 0} of dataset sample n, by the whole wave (uniform result)
__device__ __forceinline__ int wave_count_positive(const AugArgs& a, long n, int lane) {
  int L = 0;
  for (int t0 = 0; t0 < a.T; t0 += 64) {
    const int t = t0 + lane;
    L += __popcll(__ballot(t < a.T && a.time_all[(long)t * a.N + n] > 0.f));
  }
  return L;
}

// Source row of output row j of batch slot b (dataset sample n), -1 for a zero row; by the whole wave, uniform result.
__device__ __forceinline__ int wave_source_row(const AugArgs& a, const AugRates& r, int b, long n, int j, int lane) {
  const int L = wave_count_positive(a, n, lane);
  int K = 0, found = -1;
  for (int t0 = 0; t0 < L; t0 += 64) {
    const int t = t0 + lane;
    const bool kept = t < L && uniform1(r.key, SITE_FEED_TIME, (uint64_t)b * a.T + t) >= r.p_time;
    const uint64_t mask = __ballot(kept);
    const int cnt = __popcll(mask);
    if (j >= K && j < K + cnt) {                              // uniform: the pass that holds the kept row of rank j
      const bool me = kept && __popcll(mask & ((1ull << lane) - 1ull)) == j - K;
      found = t0 + __ffsll((long long)__ballot(me)) - 1;
    }
    K += cnt;
  }
  if (K == 0) return j;                                       // nothing kept (or no candidate at all): the sample stays whole
  if (j < K) return found;
  return j - K < a.T - L ? L + (j - K) : -1;
}

// lengths of batch slot b as rd_feed_gather counts it, over the times the copy workgroups write
__device__ __forceinline__ int wave_written_length(const AugArgs& a, const AugRates& r, int b, long n, int lane) {
  const int L = wave_count_positive(a, n, lane);
  int K = 0, kept_pos = 0, tail_pos = 0;
  for (int t0 = 0; t0 < a.T; t0 += 64) {
    const int t = t0 + lane;
    const bool pos = t < a.T && a.time_all[(long)t * a.N + n] > 0.f;
    const bool kept = t < L && uniform1(r.key, SITE_FEED_TIME, (uint64_t)b * a.T + t) >= r.p_time;
    K += __popcll(__ballot(kept));
    kept_pos += __popcll(__ballot(kept && pos));
    tail_pos += __popcll(__ballot(t >= L && pos));
  }
  return K == 0 ? L : kept_pos + tail_pos;
}

// steps 2 - 4 on the pair (value v, indicator m) of sensor f, source row s, slot b; kill: already dropped
__device__ __forceinline__ void finish(const AugRates& r, uint64_t elem, bool kill, float& v, float& m) {
  if (kill) { v = 0.f; m = 0.f; return; }
  if (r.noise_c != 0.f && m != 0.f) v = jitter(r, elem, v);
}

template <bool FEED>
__device__ __forceinline__ void gather_aug(AugArgs& a, const int64_t* plan, const int64_t* cell, long capacity, uint64_t draw) {
  const int tid = threadIdx.x, lane = tid & 63;
  bool ok = true;
  if (FEED) {
    const long k = feed_cursor(cell, capacity, ok);
    a.idx = plan + k * a.B;
    draw = load_uniform_u64(a.aug + 1) * (uint64_t)capacity + (uint64_t)k;
  }
  AugRates r;
  r.key = load_uniform_u64(a.aug) + draw;
  const uint64_t w2 = load_uniform_u64(a.aug + 2), w3 = load_uniform_u64(a.aug + 3);
  r.p_time = __uint_as_float((uint32_t)w2); r.p_sensor = __uint_as_float((uint32_t)(w2 >> 32));
  r.p_obs = __uint_as_float((uint32_t)w3); r.noise_c = __uint_as_float((uint32_t)(w3 >> 32));
  const bool drop_time = r.p_time > 0.f, drop_sensor = r.p_sensor > 0.f, drop_obs = r.p_obs > 0.f;

  if ((int)blockIdx.x < a.ncopy) {
    const int j = blockIdx.x / a.nbg, bg = blockIdx.x - j * a.nbg;          // j: the OUTPUT row
    const int rl = tid >> 4, l = tid & 15;
    const int b = bg * FA_RPB + rl;
    int s = j;                                                              // the SOURCE row (-1: a zero row)
    if (drop_time) {
      const int b0 = bg * FA_RPB + (tid >> 6) * 4;                          // this wave's four slots
      for (int q = 0; q < 4; ++q) {
        if (b0 + q >= a.B) break;                                          // uniform
        const int sq = wave_source_row(a, r, b0 + q, checked_index(a, b0 + q, false), j, lane);
        if (((tid >> 4) & 3) == q) s = sq;
      }
    }
    if (b >= a.B) return;
    float* d = a.src + ((long)j * a.B + b) * a.W;
    float* dm = d + a.F;
    if (s < 0) {
      if (a.vec) {
        for (int f = 2 * l; f < a.F; f += 32) {
          *reinterpret_cast<float2*>(d + f) = make_float2(0.f, 0.f);
          *reinterpret_cast<float2*>(dm + f) = make_float2(0.f, 0.f);
        }
      } else {
        for (int c = l; c < a.W; c += 16) d[c] = 0.f;
      }
      if (l == 0) a.times[(long)j * a.B + b] = 0.f;
      return;
    }
    const long n = checked_index(a, b, false);
    const float* p = a.P_all + ((long)s * a.N + n) * a.W;
    const float* pm = p + a.F;
    const uint64_t e_sensor = (uint64_t)b * a.F, e_obs = ((uint64_t)s * a.B + b) * a.F;
    if (a.vec) {
      for (int f = 2 * l; f < a.F; f += 32) {
        float2 v = *reinterpret_cast<const float2*>(p + f), m = *reinterpret_cast<const float2*>(pm + f);
        bool k0 = false, k1 = false;
        float u0, u1;
        if (drop_sensor) { uniform2(r.key, SITE_FEED_SENSOR, e_sensor + f, u0, u1); k0 = !(u0 >= r.p_sensor); k1 = !(u1 >= r.p_sensor); }
        if (drop_obs) { uniform2(r.key, SITE_FEED_OBS, e_obs + f, u0, u1); k0 = k0 || !(u0 >= r.p_obs); k1 = k1 || !(u1 >= r.p_obs); }
        finish(r, e_obs + f, k0, v.x, m.x);
        finish(r, e_obs + f + 1, k1, v.y, m.y);
        *reinterpret_cast<float2*>(d + f) = v;
        *reinterpret_cast<float2*>(dm + f) = m;
      }
    } else {
      for (int f = l; f < a.F; f += 16) {
        float v = p[f], m = pm[f];
        bool kill = drop_sensor && !(uniform1(r.key, SITE_FEED_SENSOR, e_sensor + f) >= r.p_sensor);
        if (drop_obs) kill = kill || !(uniform1(r.key, SITE_FEED_OBS, e_obs + f) >= r.p_obs);
        finish(r, e_obs + f, kill, v, m);
        d[f] = v;
        dm[f] = m;
      }
    }
    if (l == 0) a.times[(long)j * a.B + b] = a.time_all[(long)s * a.N + n];
    return;
  }
  // ---- per-sample tail, one wavefront per sample (rd_feed.hip): lengths over the WRITTEN times, label, static features ----------
  if (FEED && !ok && (int)blockIdx.x == a.ncopy && tid == 0 && a.bad) atomicAdd(a.bad, 1);   // the cursor: counted once per launch
  const int b = (blockIdx.x - a.ncopy) * 4 + (tid >> 6);
  if (b >= a.B) return;
  const long n = checked_index(a, b, lane == 0);
  const int cnt = drop_time ? wave_written_length(a, r, b, n, lane) : wave_count_positive(a, n, lane);
  if (lane == 0) {
    a.lengths[b] = (int64_t)cnt;
    if (a.y_all) a.y_out[b] = a.y_all[n];
  }
  if (a.static_all)
    for (int c = lane; c < a.ds; c += 64) a.static_out[(long)b * a.ds + c] = a.static_all[n * a.ds + c];
}

// One body, two instantiations: FEED = true is the captured step's first launch (launch-log name k_feed_gather_aug), FEED = false the
// explicit-index form (k_batch_gather_aug).
template <bool FEED>
__global__ __launch_bounds__(256) void k_gather_aug(AugArgs a, const int64_t* plan, const int64_t* cell, long capacity, uint64_t draw) {
  gather_aug<FEED>(a, plan, cell, capacity, draw);
}

int fill_args(AugArgs& a, int32_t T, int32_t B, int32_t W, int32_t d_static, int64_t N, const float* P_all, const float* time_all,
              const float* static_all, const int64_t* y_all, const int64_t* idx, float* src, float* times, float* static_out,
              int64_t* y_out, int64_t* lengths, int32_t* bad, const void* aug_cell) {
  a.P_all = P_all; a.time_all = time_all; a.static_all = d_static > 0 ? static_all : nullptr; a.y_all = y_all; a.idx = idx;
  a.src = src; a.times = times; a.static_out = static_out; a.y_out = y_out; a.lengths = lengths; a.bad = bad;
  a.aug = reinterpret_cast<const uint64_t*>(aug_cell);
  a.N = N; a.T = T; a.B = B; a.W = W; a.F = W / 2; a.ds = d_static;
  a.nbg = cdiv(B, FA_RPB);
  a.ncopy = T * a.nbg;
  // 8-byte pairs: the indicator half starts F floats behind the row, so F must be even as well as the buffers aligned
  a.vec = ((a.F & 1) == 0 && ((reinterpret_cast<uintptr_t>(P_all) | reinterpret_cast<uintptr_t>(src)) & 7) == 0) ? 1 : 0;
  return cdiv(B, 4);
}

}  // namespace
}  // namespace rd

using namespace rd;

extern "C" int rd_batch_gather_aug(int32_t T, int32_t B, int32_t W, int32_t d_static, int64_t N, const float* P_all,
                                   const float* time_all, const float* static_all, const int64_t* y_all, const int64_t* idx,
                                   float* src, float* times, float* static_out, int64_t* y_out, int64_t* lengths,
                                   int32_t* bad_index_count, const void* aug_cell, uint64_t draw, void* stream) {
  RD_REQUIRE(T >= 0 && B >= 0 && W > 0 && d_static >= 0 && N > 0, "bad dims T=%d B=%d W=%d d_static=%d N=%ld", T, B, W,
             d_static, (long)N);
  RD_REQUIRE((W & 1) == 0, "bad dims W=%d: the augmenting gather needs W = 2F (values | indicators)", W);
  if (B == 0) return RD_OK;
  RD_REQUIRE(P_all && time_all && idx && src && times && lengths && aug_cell, "NULL tensor");
  RD_REQUIRE(d_static == 0 || static_all == nullptr || static_out != nullptr, "static_all given without static_out");
  RD_REQUIRE((y_all == nullptr) == (y_out == nullptr), "y_all and y_out must be given together");
  RD_REQUIRE((reinterpret_cast<uintptr_t>(aug_cell) & 7) == 0, "aug_cell must be 8-byte aligned");
  AugArgs a{};
  const int ntail = fill_args(a, T, B, W, d_static, N, P_all, time_all, static_all, y_all, idx, src, times, static_out, y_out, lengths,
                              bad_index_count, aug_cell);
  hipLaunchKernelGGL(k_gather_aug<false>, dim3(a.ncopy + ntail), dim3(256), 0, (hipStream_t)stream, a, (const int64_t*)nullptr,
                     (const int64_t*)nullptr, 0L, draw);
  return check_launch("k_batch_gather_aug");
}

extern "C" int rd_feed_gather_aug(int32_t T, int32_t B, int32_t W, int32_t d_static, int64_t N, int64_t capacity, const float* P_all,
                                  const float* time_all, const float* static_all, const int64_t* y_all, const int64_t* plan,
                                  const int64_t* cell, float* src, float* times, float* static_out, int64_t* y_out,
                                  int64_t* lengths, int32_t* bad_index_count, const void* aug_cell, void* stream) {
  RD_REQUIRE(T >= 0 && B >= 0 && W > 0 && d_static >= 0 && N > 0 && capacity > 0, "bad dims T=%d B=%d W=%d d_static=%d N=%ld capacity=%ld",
             T, B, W, d_static, (long)N, (long)capacity);
  RD_REQUIRE((W & 1) == 0, "bad dims W=%d: the augmenting gather needs W = 2F (values | indicators)", W);
  if (B == 0) return RD_OK;
  RD_REQUIRE(P_all && time_all && y_all && plan && cell && src && times && y_out && lengths && aug_cell, "NULL tensor");
  RD_REQUIRE(d_static == 0 || static_all == nullptr || static_out != nullptr, "static_all given without static_out");
  RD_REQUIRE((reinterpret_cast<uintptr_t>(aug_cell) & 7) == 0, "aug_cell must be 8-byte aligned");
  AugArgs a{};
  const int ntail = fill_args(a, T, B, W, d_static, N, P_all, time_all, static_all, y_all, nullptr, src, times, static_out, y_out,
                              lengths, bad_index_count, aug_cell);
  hipLaunchKernelGGL(k_gather_aug<true>, dim3(a.ncopy + ntail), dim3(256), 0, (hipStream_t)stream, a, plan, cell, (long)capacity,
                     (uint64_t)0);
  return check_launch("k_feed_gather_aug");
}
