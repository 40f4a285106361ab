// Per-cluster sums and means of feature rows: the update half of a Lloyd (k-means) iteration, on the device and without atomics on
// floats.  The assignment half is jck_knn_index_f32 with k = 1.
//
//   jck_segment_mean_f32    sum[c] = the sum of the rows of x[N][D] with label c, count[c] their number, centre[c] = sum[c] / count[c]
//   jck_segment_ws_bytes    its workspace (host only)
//   jck_segment_chunk_rows  R, the rows of one piece (host only)
//
// The order of every addition is fixed by the labels alone.  Five launches:
//   histogram   seg_hist_kernel: the rows are cut into strips, one wave per strip counts its strip's labels in LDS (integer adds).
//   scan        seg_scan_kernel, one workgroup: per cluster the strips' counts become the places where each strip's rows of that cluster
//               go in the sorted list (a stable counting sort: clusters in ascending order, inside a cluster the rows in ascending
//               index), count[] is written, every cluster's list is cut FROM ITS OWN START into pieces of R = 64 rows and the pieces are
//               numbered, cluster after cluster.
//   scatter     seg_scatter_kernel, one wave per strip: 64 rows at a time, a row's place is its strip's cursor of the label plus the
//               number of lower lanes with the same label.
//   pieces      seg_piece_kernel, the pass over x: one workgroup per (piece, 256 threads' columns); a thread owns one float4 of
//               columns (one float on the scalar path) and adds the piece's rows to it in list order, eight row loads in flight.  A wave
//               reads 1 KiB of a row per instruction; every element of x is read once.  The partial goes to the workspace.
//   final       seg_final_kernel: a cluster's partials are added in ascending piece order; sum, and centre where count > 0, leave.
// So sum[c] = (((p_0 + p_1) + p_2) + ...) with p_j = ((((0 + r_64j) + r_64j+1) + ...): a function of the sequence of rows labelled c
// and of nothing else - not of N, K, the other rows, the grid or the order in which workgroups ran.  A K x columns table in LDS would
// need LDS float atomics to be fast (the order of arrival would decide the bits) and does not hold K = 1024 rows of any useful width.
// Labels outside 0 .. K-1 are skipped: they are in no histogram, so they are in no list.
#include "pairtile.hpp"

namespace {

constexpr int SEG_R = 64;                 // rows of a piece
constexpr int SEG_UNROLL = 8;             // row loads in flight per thread
constexpr int SEG_KMAX = 1024;
constexpr int SEG_STRIP_MIN = 256;        // rows of a strip at least; at most SEG_STRIPS_MAX strips
constexpr int SEG_STRIPS_MAX = 1024;
constexpr int SEG_COLS = 256;             // threads of a piece workgroup: 256 float4s (vector path) or floats of columns
constexpr long long SEG_D_MAX = 65535LL * SEG_COLS;      // grid.y of the scalar path

struct SegP {
  const float* x; const long long* label;
  int N, D, K, strip, nstrips, pmax;
  int* hist;            // [nstrips][K]: counts, then (scan) the first place of the strip's rows of cluster c in `sorted`
  int* start;           // [K + 1]: cluster c's list is sorted[start[c] .. start[c + 1])
  int* pstart;          // [K + 1]: cluster c's pieces are pstart[c] .. pstart[c + 1); pstart[K] = pieces in all
  int* pcl;             // [pmax]: the cluster of a piece
  int* sorted;          // [N]: row indices by (label, index); the tail past start[K] is unused
  float* part;          // [pmax][D]: the pieces' sums
  float* sum; int* count; float* centre;
};

inline int seg_strip_of(int N) {
  const long long per = ((long long)N + SEG_STRIPS_MAX - 1) / SEG_STRIPS_MAX;
  return (int)std::max<long long>(SEG_STRIP_MIN, (per + 63) / 64 * 64);
}
inline int seg_strips_of(int N) { const int s = seg_strip_of(N); return (int)(((long long)N + s - 1) / s); }
// pieces at most: every cluster's last piece may be short
inline long long seg_pmax_of(int N, int K) { return (long long)N / SEG_R + std::min(N, K); }
inline bool seg_sizes_ok(int N, long long D, int K) { return N >= 1 && N <= P_MAX_ROWS && D >= 1 && D <= SEG_D_MAX && K >= 1 && K <= SEG_KMAX; }

__global__ __launch_bounds__(64) void seg_hist_kernel(const SegP p) {
  __shared__ int h[SEG_KMAX];
  const int lane = threadIdx.x;
  for (int c = lane; c < p.K; c += 64) h[c] = 0;
  __syncthreads();
  const long long r0 = (long long)blockIdx.x * p.strip, r1 = r0 + p.strip < p.N ? r0 + p.strip : p.N;
  for (long long r = r0 + lane; r < r1; r += 64) {
    const long long l = p.label[r];
    if (l >= 0 && l < p.K) atomicAdd(&h[(int)l], 1);
  }
  __syncthreads();
  for (int c = lane; c < p.K; c += 64) p.hist[(long long)blockIdx.x * p.K + c] = h[c];
}

__global__ __launch_bounds__(SEG_KMAX) void seg_scan_kernel(const SegP p) {
  __shared__ int st[SEG_KMAX + 1], ps[SEG_KMAX + 1];
  const int c = threadIdx.x;
  int total = 0;
  if (c < p.K) {
    for (int s = 0; s < p.nstrips; ++s) total += p.hist[(long long)s * p.K + c];
    st[c] = total;
  }
  __syncthreads();
  if (c == 0) {
    int rows = 0, pieces = 0;
    for (int k = 0; k < p.K; ++k) {
      const int n = st[k];
      st[k] = rows; ps[k] = pieces;
      rows += n; pieces += (n + SEG_R - 1) / SEG_R;
    }
    st[p.K] = rows; ps[p.K] = pieces;
  }
  __syncthreads();
  if (c < p.K) {
    p.count[c] = total;
    p.start[c] = st[c];
    p.pstart[c] = ps[c];
    int run = st[c];
    for (int s = 0; s < p.nstrips; ++s) {
      const long long o = (long long)s * p.K + c;
      const int n = p.hist[o];
      p.hist[o] = run;
      run += n;
    }
  }
  if (c == 0) { p.start[p.K] = st[p.K]; p.pstart[p.K] = ps[p.K]; }
  const int pieces = ps[p.K] < p.pmax ? ps[p.K] : p.pmax;                  // (never more than pmax: seg_pmax_of)
  for (int q = c; q < pieces; q += SEG_KMAX) {                             // the smallest cluster whose pieces end past q
    int lo = 0, hi = p.K - 1;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (ps[mid + 1] <= q) lo = mid + 1; else hi = mid;
    }
    p.pcl[q] = lo;
  }
}

__global__ __launch_bounds__(64) void seg_scatter_kernel(const SegP p) {
  __shared__ int cur[SEG_KMAX];
  const int lane = threadIdx.x;
  for (int c = lane; c < p.K; c += 64) cur[c] = p.hist[(long long)blockIdx.x * p.K + c];
  __syncthreads();
  const long long r0 = (long long)blockIdx.x * p.strip, r1 = r0 + p.strip < p.N ? r0 + p.strip : p.N;
  for (long long base = r0; base < r1; base += 64) {                       // wave-uniform
    const long long r = base + lane;
    int lab = -1;
    if (r < r1) {
      const long long l = p.label[r];
      if (l >= 0 && l < p.K) lab = (int)l;
    }
    int rank = 0, total = 0;                                               // lower lanes / all lanes of this label
#pragma unroll 8
    for (int j = 0; j < 64; ++j) {
      const int same = __shfl(lab, j, 64) == lab ? 1 : 0;
      total += same;
      rank += j < lane ? same : 0;
    }
    if (lab >= 0) {
      const int pos = cur[lab] + rank;
      if (pos < p.N) p.sorted[pos] = (int)r;
    }
    __syncthreads();
    if (lab >= 0 && rank == total - 1) cur[lab] += total;
    __syncthreads();
  }
}

template <int V> struct SegVec;
template <> struct SegVec<4> { typedef f32x4 T; static __device__ __forceinline__ T zero() { return f32x4{0.f, 0.f, 0.f, 0.f}; } };
template <> struct SegVec<1> { typedef float T; static __device__ __forceinline__ T zero() { return 0.f; } };

// the sum of one piece's rows over this workgroup's columns, in list order
template <int V> __global__ __launch_bounds__(SEG_COLS) void seg_piece_kernel(const SegP p) {
  typedef typename SegVec<V>::T T;
  const int piece = (int)blockIdx.x;
  if (piece >= p.pstart[p.K]) return;
  const int c = p.pcl[piece];
  const int first = p.start[c] + (piece - p.pstart[c]) * SEG_R;
  const int left = p.start[c + 1] - first, n = left < SEG_R ? left : SEG_R;
  const long long col = ((long long)blockIdx.y * SEG_COLS + threadIdx.x) * V;
  if (col >= p.D) return;                                                  // V == 4: D % 4 == 0, so col + 3 < D
  const int* __restrict__ rows = p.sorted + first;
  const float* __restrict__ xc = p.x + col;
  T acc = SegVec<V>::zero();
  int i = 0;
  for (; i + SEG_UNROLL <= n; i += SEG_UNROLL) {
    T v[SEG_UNROLL];
#pragma unroll
    for (int u = 0; u < SEG_UNROLL; ++u) v[u] = *reinterpret_cast<const T*>(xc + (long long)rows[i + u] * p.D);
#pragma unroll
    for (int u = 0; u < SEG_UNROLL; ++u) acc += v[u];
  }
  for (; i < n; ++i) acc += *reinterpret_cast<const T*>(xc + (long long)rows[i] * p.D);
  *reinterpret_cast<T*>(p.part + (long long)piece * p.D + col) = acc;
}

__device__ __forceinline__ float seg_div(float s, float n) { return __fdiv_rn(s, n); }
__device__ __forceinline__ f32x4 seg_div(f32x4 s, float n) { return f32x4{__fdiv_rn(s[0], n), __fdiv_rn(s[1], n), __fdiv_rn(s[2], n), __fdiv_rn(s[3], n)}; }

// a cluster's pieces in ascending order -> sum, centre
template <int V> __global__ __launch_bounds__(SEG_COLS) void seg_final_kernel(const SegP p) {
  typedef typename SegVec<V>::T T;
  const int c = (int)blockIdx.x;
  const long long col = ((long long)blockIdx.y * SEG_COLS + threadIdx.x) * V;
  if (col >= p.D) return;
  const int q0 = p.pstart[c], q1 = p.pstart[c + 1], cnt = p.start[c + 1] - p.start[c];
  T acc = SegVec<V>::zero();
#pragma unroll 4
  for (int q = q0; q < q1; ++q) acc += *reinterpret_cast<const T*>(p.part + (long long)q * p.D + col);
  *reinterpret_cast<T*>(p.sum + (long long)c * p.D + col) = acc;
  if (p.centre && cnt > 0) *reinterpret_cast<T*>(p.centre + (long long)c * p.D + col) = seg_div(acc, (float)cnt);
}

inline size_t seg_up16(size_t b) { return (b + 15) & ~(size_t)15; }
// the histogram's share of the workspace is sized by a bound on the strips that grows with N (the strips themselves do not)
inline size_t seg_hist_rows(int N) { return (size_t)std::min<long long>(SEG_STRIPS_MAX, ((long long)N + SEG_STRIP_MIN - 1) / SEG_STRIP_MIN); }

}  // namespace

extern "C" int jck_segment_chunk_rows(void) { return SEG_R; }

extern "C" size_t jck_segment_ws_bytes(int N, int D, int K) {
  if (!seg_sizes_ok(N, D, K)) return 0;
  const size_t pmax = (size_t)seg_pmax_of(N, K);
  return seg_up16(pmax * (size_t)D * sizeof(float)) + seg_up16((seg_hist_rows(N) * (size_t)K + 2 * ((size_t)K + 1) + pmax + (size_t)N) * sizeof(int));
}

extern "C" int jck_segment_mean_f32(const float* x, int N, int D, const long long* label, int K, float* sum, int* count, float* centre,
                                    void* ws, void* stream) {
  if (!x || !label || !sum || !count || !ws) JCK_FAIL(JCK_E_ARG, "segment_mean: null argument");
  if (K < 1 || K > SEG_KMAX) JCK_FAIL(JCK_E_ARG, "segment_mean: K must be 1..1024");
  if (!seg_sizes_ok(N, D, K)) JCK_FAIL(JCK_E_ARG, "segment_mean: bad sizes");
  SegP p = {};
  p.x = x; p.label = label; p.N = N; p.D = D; p.K = K; p.sum = sum; p.count = count; p.centre = centre;
  p.strip = seg_strip_of(N); p.nstrips = seg_strips_of(N); p.pmax = (int)seg_pmax_of(N, K);
  p.part = (float*)ws;
  p.hist = (int*)((char*)ws + seg_up16((size_t)p.pmax * (size_t)D * sizeof(float)));
  p.start = p.hist + seg_hist_rows(N) * (size_t)K;
  p.pstart = p.start + (K + 1);
  p.pcl = p.pstart + (K + 1);
  p.sorted = p.pcl + p.pmax;
  // 16-byte path: whole float4s in every row, and every base the float4s are read from or written to on a 16-byte boundary
  const int vec = D % 4 == 0 && (((uintptr_t)x | (uintptr_t)sum | (uintptr_t)centre | (uintptr_t)ws) & 15) == 0;
  const hipStream_t st = (hipStream_t)stream;
  const unsigned tiles = (unsigned)(((long long)D + SEG_COLS * (vec ? 4 : 1) - 1) / (SEG_COLS * (vec ? 4 : 1)));
  hipLaunchKernelGGL(seg_hist_kernel, dim3((unsigned)p.nstrips), dim3(64), 0, st, p);
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(seg_scan_kernel, dim3(1), dim3(SEG_KMAX), 0, st, p);
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(seg_scatter_kernel, dim3((unsigned)p.nstrips), dim3(64), 0, st, p);
  HIPCHK(hipGetLastError());
  if (vec) {
    hipLaunchKernelGGL(seg_piece_kernel<4>, dim3((unsigned)p.pmax, tiles), dim3(SEG_COLS), 0, st, p);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(seg_final_kernel<4>, dim3((unsigned)K, tiles), dim3(SEG_COLS), 0, st, p);
  } else {
    hipLaunchKernelGGL(seg_piece_kernel<1>, dim3((unsigned)p.pmax, tiles), dim3(SEG_COLS), 0, st, p);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(seg_final_kernel<1>, dim3((unsigned)K, tiles), dim3(SEG_COLS), 0, st, p);
  }
  HIPCHK(hipGetLastError());
  return JCK_OK;
}
