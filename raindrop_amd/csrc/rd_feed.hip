// rd_feed.hip -- batch feed from a device-resident dataset.
//
// Replaces the per-step host fancy-index + H2D of code/Raindrop.py:310-315
//   P, Ptime, Pstatic, y = Ptrain_tensor[:, idx, :].cuda(), Ptrain_time_tensor[:, idx].cuda(),
//                          Ptrain_static_tensor[idx].cuda(), ytrain_tensor[idx].cuda()
// and `lengths = torch.sum(Ptime > 0, dim=0)` (:317) with ONE launch over tensors that already live in
// HBM: pure byte movement (bit-exact), bound by HBM: 2 * B * T * (W + 1) * 4 bytes per batch
// (P19, B=256: 8.5 MB -> 1.1 us at 8 TB/s).
#include "rd_common.h"

namespace rd {
namespace {

constexpr int FD_RPB = 16;        // batch rows per copy workgroup: 16 rows x 16 lanes x 16 bytes per pass

struct FeedArgs {
  const float *P_all, *time_all, *static_all;
  const int64_t *y_all, *idx;
  float *src, *times, *static_out;
  int64_t *y_out, *lengths;
  int32_t* bad;
  long N;
  int T, B, W, ds, ncopy, nbg, vec;
};

// an out-of-range index is counted (integer atomic) and clamped; the caller decides what to do with the count
__device__ __forceinline__ long checked_index(const FeedArgs& a, int b, bool count) {
  long n = a.idx[b];
  if (n < 0 || n >= a.N) {
    if (count && a.bad) atomicAdd(a.bad, 1);
    n = n < 0 ? 0 : a.N - 1;
  }
  return n;
}

__global__ __launch_bounds__(256) void k_batch_gather(FeedArgs a) {
  const int tid = threadIdx.x;
  if ((int)blockIdx.x < a.ncopy) {
    // ---- [T, N, W] -> [T, B, W] rows and [T, N] -> [T, B] time stamps -----------------------------------
    const int t = blockIdx.x / a.nbg, bg = blockIdx.x - t * a.nbg;
    const int r = tid >> 4, l = tid & 15;
    const int b = bg * FD_RPB + r;
    if (b >= a.B) return;
    const long n = checked_index(a, b, false);
    const float* s = a.P_all + ((long)t * a.N + n) * a.W;
    float* d = a.src + ((long)t * a.B + b) * a.W;
    if (a.vec) {
      for (int c = 4 * l; c < a.W; c += 64) *reinterpret_cast<float4*>(d + c) = *reinterpret_cast<const float4*>(s + c);
    } else {
      for (int c = l; c < a.W; c += 16) d[c] = s[c];
    }
    if (l == 0) a.times[(long)t * a.B + b] = a.time_all[(long)t * a.N + n];
    return;
  }
  // ---- per-sample tail, one wavefront per sample: lengths (code/Raindrop.py:317) as a wave-wide count over
  // the time axis (one round trip instead of a T-long dependent loop), labels, static features -------------
  const int lane = tid & 63;
  const int b = (blockIdx.x - a.ncopy) * 4 + (tid >> 6);
  if (b >= a.B) return;
  const long n = checked_index(a, b, lane == 0);
  int cnt = 0;
  for (int t = lane; t < a.T; t += 64) cnt += a.time_all[(long)t * a.N + n] > 0.f ? 1 : 0;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
  if (lane == 0) {
    a.lengths[b] = (int64_t)cnt;
    if (a.y_all) a.y_out[b] = a.y_all[n];
  }
  if (a.static_all)
    for (int j = lane; j < a.ds; j += 64) a.static_out[(long)b * a.ds + j] = a.static_all[n * a.ds + j];
}

// ---- the batch of a captured step, drawn from a device-resident epoch plan -------------------------------------------------
// cell = {cursor, n_batches} (int64[2]), read through the scalar cache when the kernel RUNS (uniform: every workgroup asks for
// the same 16 bytes): a replay of the same graph gathers the next batch.  The step's last launch (k_feed_record) advances the
// cursor; nothing here writes it.  The row actually read always lies inside the plan: n_batches is cut to the plan's capacity,
// a cursor outside [0, n_batches) is replaced by the last valid row (row 0 of an empty plan) and reported by `bad`.
__device__ __forceinline__ long feed_cursor(const int64_t* cell, long capacity, bool& ok) {
  const long k = (long)load_uniform_u64(reinterpret_cast<const uint64_t*>(cell));
  long nb = (long)load_uniform_u64(reinterpret_cast<const uint64_t*>(cell + 1));
  nb = nb < capacity ? nb : capacity;
  ok = k >= 0 && k < nb;
  return ok ? k : (nb > 0 ? nb - 1 : 0);
}

// k_batch_gather with idx = plan[cursor]: the same copies, workgroup for workgroup
__global__ __launch_bounds__(256) void k_feed_gather(FeedArgs a, const int64_t* plan, const int64_t* cell, long capacity) {
  const int tid = threadIdx.x;
  bool ok;
  a.idx = plan + feed_cursor(cell, capacity, ok) * a.B;
  if ((int)blockIdx.x < a.ncopy) {
    const int t = blockIdx.x / a.nbg, bg = blockIdx.x - t * a.nbg;
    const int r = tid >> 4, l = tid & 15;
    const int b = bg * FD_RPB + r;
    if (b >= a.B) return;
    const long n = checked_index(a, b, false);
    const float* s = a.P_all + ((long)t * a.N + n) * a.W;
    float* d = a.src + ((long)t * a.B + b) * a.W;
    if (a.vec) {
      for (int c = 4 * l; c < a.W; c += 64) *reinterpret_cast<float4*>(d + c) = *reinterpret_cast<const float4*>(s + c);
    } else {
      for (int c = l; c < a.W; c += 16) d[c] = s[c];
    }
    if (l == 0) a.times[(long)t * a.B + b] = a.time_all[(long)t * a.N + n];
    return;
  }
  if (!ok && (int)blockIdx.x == a.ncopy && tid == 0 && a.bad) atomicAdd(a.bad, 1);   // the cursor: counted once per launch
  const int lane = tid & 63;
  const int b = (blockIdx.x - a.ncopy) * 4 + (tid >> 6);
  if (b >= a.B) return;
  const long n = checked_index(a, b, lane == 0);
  int cnt = 0;
  for (int t = lane; t < a.T; t += 64) cnt += a.time_all[(long)t * a.N + n] > 0.f ? 1 : 0;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
  if (lane == 0) {
    a.lengths[b] = (int64_t)cnt;
    a.y_out[b] = a.y_all[n];
  }
  if (a.static_all)
    for (int j = lane; j < a.ds; j += 64) a.static_out[(long)b * a.ds + j] = a.static_all[n * a.ds + j];
}

// The step's last launch, ONE workgroup: loss_hist[k] = *loss, correct_hist[k] = #{b : argmax_c logits[b, c] == y[b]} (the first
// maximum wins, a NaN counts as the maximum: torch.argmax), cursor = k + 1.  Integer partial counts summed wave by wave in a
// fixed order, no atomics.  The cursor is read by every thread in front of the barrier and written by thread 0 behind it; the
// next reader is the next step's first launch, in stream order.  A cursor outside [0, n_batches): nothing is written.
__global__ __launch_bounds__(256) void k_feed_record(int64_t* cell, long capacity, const float* loss, const float* logits,
                                                     const int64_t* y, float* loss_hist, int32_t* correct_hist, int B, int C) {
  __shared__ int part[4];
  const int tid = threadIdx.x;
  bool ok;
  const long k = feed_cursor(cell, capacity, ok);
  if (!ok) return;                                          // uniform
  int cnt = 0;
  for (int b = tid; b < B; b += 256) {
    const float* row = logits + (long)b * C;
    float best = row[0];
    int arg = 0;
    for (int c = 1; c < C; ++c) {
      const float v = row[c];
      if (v > best || (v != v && best == best)) { best = v; arg = c; }
    }
    cnt += (int64_t)arg == y[b] ? 1 : 0;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
  if ((tid & 63) == 0) part[tid >> 6] = cnt;
  __syncthreads();
  if (tid == 0) {
    loss_hist[k] = *loss;
    correct_hist[k] = part[0] + part[1] + part[2] + part[3];
    cell[0] = k + 1;
  }
}

}  // namespace
}  // namespace rd

using namespace rd;

extern "C" int rd_batch_gather(int32_t T, int32_t B, int32_t W, int32_t d_static, int64_t N, const float* P_all,
                               const float* time_all, const float* static_all, const int64_t* y_all,
                               const int64_t* idx, float* src, float* times, float* static_out, int64_t* y_out,
                               int64_t* lengths, int32_t* bad_index_count, void* stream) {
  RD_REQUIRE(T >= 0 && B >= 0 && W > 0 && d_static >= 0 && N > 0, "bad dims T=%d B=%d W=%d d_static=%d N=%ld", T, B, W,
             d_static, (long)N);
  hipStream_t st = (hipStream_t)stream;
  if (B == 0) return RD_OK;
  RD_REQUIRE(P_all && time_all && idx && src && times && lengths, "NULL tensor");
  RD_REQUIRE(d_static == 0 || static_all == nullptr || static_out != nullptr, "static_all given without static_out");
  RD_REQUIRE((y_all == nullptr) == (y_out == nullptr), "y_all and y_out must be given together");
  FeedArgs a{};
  a.P_all = P_all; a.time_all = time_all; a.static_all = d_static > 0 ? static_all : nullptr; a.y_all = y_all; a.idx = idx;
  a.src = src; a.times = times; a.static_out = static_out; a.y_out = y_out; a.lengths = lengths; a.bad = bad_index_count;
  a.N = N; a.T = T; a.B = B; a.W = W; a.ds = d_static;
  a.nbg = cdiv(B, FD_RPB);
  a.ncopy = T * a.nbg;
  a.vec = ((W & 3) == 0 && ((reinterpret_cast<uintptr_t>(P_all) | reinterpret_cast<uintptr_t>(src)) & 15) == 0) ? 1 : 0;
  const int ntail = cdiv(B, 4);
  hipLaunchKernelGGL(k_batch_gather, dim3(a.ncopy + ntail), dim3(256), 0, st, a);
  return check_launch("k_batch_gather");
}

extern "C" int rd_feed_gather(int32_t T, int32_t B, int32_t W, int32_t d_static, int64_t N, int64_t capacity, const float* P_all,
                              const float* time_all, const float* static_all, const int64_t* y_all, const int64_t* plan,
                              const int64_t* cell, float* src, float* times, float* static_out, int64_t* y_out, int64_t* lengths,
                              int32_t* bad_index_count, void* stream) {
  RD_REQUIRE(T >= 0 && B >= 0 && W > 0 && d_static >= 0 && N > 0 && capacity > 0, "bad dims T=%d B=%d W=%d d_static=%d N=%ld capacity=%ld",
             T, B, W, d_static, (long)N, (long)capacity);
  hipStream_t st = (hipStream_t)stream;
  if (B == 0) return RD_OK;
  RD_REQUIRE(P_all && time_all && y_all && plan && cell && src && times && y_out && lengths, "NULL tensor");
  RD_REQUIRE(d_static == 0 || static_all == nullptr || static_out != nullptr, "static_all given without static_out");
  FeedArgs a{};
  a.P_all = P_all; a.time_all = time_all; a.static_all = d_static > 0 ? static_all : nullptr; a.y_all = y_all; a.idx = nullptr;
  a.src = src; a.times = times; a.static_out = static_out; a.y_out = y_out; a.lengths = lengths; a.bad = bad_index_count;
  a.N = N; a.T = T; a.B = B; a.W = W; a.ds = d_static;
  a.nbg = cdiv(B, FD_RPB);
  a.ncopy = T * a.nbg;
  a.vec = ((W & 3) == 0 && ((reinterpret_cast<uintptr_t>(P_all) | reinterpret_cast<uintptr_t>(src)) & 15) == 0) ? 1 : 0;
  const int ntail = cdiv(B, 4);
  hipLaunchKernelGGL(k_feed_gather, dim3(a.ncopy + ntail), dim3(256), 0, st, a, plan, cell, (long)capacity);
  return check_launch("k_feed_gather");
}

extern "C" int rd_feed_record(int32_t B, int32_t C, int64_t capacity, int64_t* cell, const float* loss, const float* logits,
                              const int64_t* y, float* loss_hist, int32_t* correct_hist, void* stream) {
  RD_REQUIRE(B >= 0 && C > 0 && capacity > 0, "bad dims B=%d C=%d capacity=%ld", B, C, (long)capacity);
  if (B == 0) return RD_OK;
  RD_REQUIRE(cell && loss && logits && y && loss_hist && correct_hist, "NULL tensor");
  hipLaunchKernelGGL(k_feed_record, dim3(1), dim3(256), 0, (hipStream_t)stream, cell, (long)capacity, loss, logits, y, loss_hist,
                     correct_hist, B, C);
  return check_launch("k_feed_record");
}
