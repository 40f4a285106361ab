// Nearest reference rows of query rows, WITH their indices (memorisation checks: each sample beside its nearest training images).
//
//   jck_knn_index_f32       idx[i][0..k) / d2[i][0..k) = the k reference rows nearest to q_i, ascending by (d2, index)
//   jck_knn_index_ws_bytes  its workspace (host only)
//
// Two stages, two launches, both on the device:
//   candidates  knn_cand_kernel: the Gram-tile core of pairtile.hpp with the queries as the workgroup's own block (tile columns) and
//               the references walked (tile rows).  d = max(0, (|ref|^2 + |q|^2) - 2 G) in fp32.  A lane keeps, for each of its two
//               query columns, the 8 smallest (d, reference row) pairs in lexicographic order; the 8 lanes that share a column
//               merge once through LDS.
//               The walk is split: the grid is (query tiles x strips of reference tiles), every workgroup writes its 64 x 8 partial
//               lists to the workspace.  No atomics: the partial lists have fixed places, every merge compares (d, index) pairs,
//               whose order is total, so the 8 survivors do not depend on the order in which anything ran.
//   ranks       knn_rank_kernel, one wave per query: the strips' lists merge to the 8 candidates (per-lane lists, then 8 rounds of
//               a wave-wide lexicographic minimum), each candidate's distance is recomputed from differences, sum_c (q_c - ref_c)^2
//               (fp32: a fmaf chain per lane over c = lane, lane + 64, ..., or over float4s of c, then a butterfly over the lanes -
//               a fixed order of non-negative terms, so |d2 - exact| <= (D + 4) 2^-24 exact), the candidates and, with `merge`,
//               the caller's earlier results sort by (d2, global index) and the first k leave.
// Why two stages: the Gram form has an ABSOLUTE error of about 3 (D + 2) 2^-24 (|q|^2 + |ref|^2); for a near copy at D = 12 288 that
// is 10^-1 where d2 is 10^-2.  It is good enough to pick 8 candidates, not to rank or report them.
// Non-finite values: a NaN distance compares false everywhere, so a reference row with a non-finite norm is never kept; a query
// row with a non-finite norm keeps nothing and leaves with idx -1 / d2 NaN.
#include "pairtile.hpp"

namespace {

constexpr int KNN_WGS = 768;              // workgroups the candidate walk is split into at least (3 per CU of 256) where the tiles allow
constexpr int KSUB = 4;                   // 16-column steps of the tile core staged per barrier pair

struct KnnCandP {
  const float* q; const float* ref;
  int M, N, D, vec, strip, nstrips, exclude;
  long long self_off;                     // q_base - ref_base: query row i is reference row i + self_off
  float* qn; float* cd; int* ci;          // workspace: query norms [M], partial lists [M][nstrips][8]
};

struct KnnRankP {
  const float* q; const float* ref;
  int M, D, vec, k, nstrips, merge;
  long long ref_base;
  const float* qn; const float* cd; const int* ci;
  long long* idx; float* d2;
};

__global__ __launch_bounds__(256) void knn_cand_kernel(const KnnCandP p) {
  // KSUB staged steps of the tile core per barrier pair: their global loads are in flight together.  After the walk the same
  // memory holds the lists that the lanes of a column merge (8 lanes x 8 entries x 64 columns of distances, then of indices).
  __shared__ __attribute__((aligned(16))) float smem[2 * KSUB * PT * PLD];
  __shared__ float nA[PT], nB[PT];
  float (*As)[PT][PLD] = reinterpret_cast<float (*)[PT][PLD]>(smem);
  float (*Bs)[PT][PLD] = As + KSUB;
  float* candD = smem;
  int* candI = reinterpret_cast<int*>(smem + PT * 8 * PKMAX);
  static_assert(2 * PT * 8 * PKMAX <= 2 * KSUB * PT * PLD, "the merge lists fit the staging memory");
  const TilePos t(threadIdx.x);
  const int tid = t.tid;
  const int b0 = (int)blockIdx.x * PT;                                  // the query block
  const long long tilesA = ((long long)p.N + PT - 1) / PT;
  const long long t0 = (long long)blockIdx.y * p.strip, t1 = t0 + p.strip < tilesA ? t0 + p.strip : tilesA;
  TopK<true> L[2];
  int self[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    L[j].clear();
    const long long s = (long long)(b0 + t.col(j)) + p.self_off;
    self[j] = (p.exclude && s >= 0 && s < p.N) ? (int)s : -1;
  }

  for (long long ta = t0; ta < t1; ++ta) {
    const int a0 = (int)(ta * PT);
    f32x4 acc[2][2];
    gram_tile<KSUB, true>(acc, As, Bs, nA, nB, p.ref, p.N, a0, p.q, p.M, b0, p.D, p.vec, ta == t0, t);
    __syncthreads();
    // a lane meets its references in ascending order
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const float nb = nB[t.col(j)];
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int ra = t.row(i, r), ga = a0 + ra;
          float d = (nA[ra] + nb) - 2.f * acc[i][j][r];
          d = d < 0.f ? 0.f : d;                                        // NaN stays NaN and is never kept
          if (ga < p.N && ga != self[j]) L[j].offer(d, ga);
        }
    }
  }

  TopK<true> M;
  merge_columns(M, L, candD, candI, t);
  if (tid < PT && b0 + tid < p.M) {
    const long long o = ((long long)(b0 + tid) * p.nstrips + blockIdx.y) * PKMAX;
#pragma unroll
    for (int e = 0; e < PKMAX; ++e) { p.cd[o + e] = M.v[e]; p.ci[o + e] = M.i[e]; }
    if (blockIdx.y == 0) p.qn[b0 + tid] = nB[tid];
  }
}

__device__ __forceinline__ float wave_sum_f(float v) {                  // butterfly: every lane ends with the same bits
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// one wave per query row: merge the strips' lists, recompute the candidates' distances from differences, sort, write k
__global__ __launch_bounds__(256) void knn_rank_kernel(const KnnRankP p) {
  const int lane = threadIdx.x & 63;
  const long long qrow = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (qrow >= p.M) return;                                              // wave-uniform; no workgroup barrier below
  TopK<true> L;
  L.clear();
  const long long base = qrow * p.nstrips * PKMAX;
  const int n = p.nstrips * PKMAX;
  for (int e = lane; e < n; e += 64) L.offer(p.cd[base + e], p.ci[base + e]);
  // 8 rounds: the smallest head of the 64 sorted lists leaves its list.  Real entries are distinct (one per reference row); padding
  // entries are all alike, and a list that pops one only shifts in another.
  float C[PKMAX];
  int CI[PKMAX];
#pragma unroll
  for (int t = 0; t < PKMAX; ++t) {
    float hd = L.v[0];
    int hi = L.i[0];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float od = __shfl_xor(hd, o, 64);
      const int oi = __shfl_xor(hi, o, 64);
      const bool lt = TopK<true>::less(od, oi, hd, hi);
      hd = lt ? od : hd;
      hi = lt ? oi : hi;
    }
    C[t] = hd; CI[t] = hi;
    if (L.v[0] == hd && L.i[0] == hi) L.pop();
  }
  // distances from differences; a padding candidate reads reference row 0 and is dropped below
  const float* __restrict__ qr = p.q + qrow * p.D;
  const float* rr[PKMAX];
  float acc[PKMAX];
#pragma unroll
  for (int t = 0; t < PKMAX; ++t) {
    rr[t] = p.ref + (long long)(C[t] < INFINITY ? CI[t] : 0) * p.D;
    acc[t] = 0.f;
  }
  if (p.vec) {
#pragma unroll 2
    for (int c = lane * 4; c < p.D; c += 256) {
      const f32x4 qv = *reinterpret_cast<const f32x4*>(qr + c);
#pragma unroll
      for (int t = 0; t < PKMAX; ++t) {
        const f32x4 rv = *reinterpret_cast<const f32x4*>(rr[t] + c);
#pragma unroll
        for (int e = 0; e < 4; ++e) { const float dv = qv[e] - rv[e]; acc[t] = fmaf(dv, dv, acc[t]); }
      }
    }
  } else {
    for (int c = lane; c < p.D; c += 64) {
      const float qv = qr[c];
#pragma unroll
      for (int t = 0; t < PKMAX; ++t) { const float dv = qv - rr[t][c]; acc[t] = fmaf(dv, dv, acc[t]); }
    }
  }
  // lanes 0..7: the candidates; lanes 8..15: the caller's earlier results (merge); a padding key is (+inf, max)
  float kd = INFINITY;
  long long ki = 0x7fffffffffffffffLL;
#pragma unroll
  for (int t = 0; t < PKMAX; ++t) {
    const float s = wave_sum_f(acc[t]);
    if (lane == t && C[t] < INFINITY && s < INFINITY) { kd = s; ki = p.ref_base + CI[t]; }
  }
  if (p.merge && lane >= PKMAX && lane < PKMAX + p.k) {
    const long long gi = p.idx[qrow * p.k + (lane - PKMAX)];
    const float gd = p.d2[qrow * p.k + (lane - PKMAX)];
    if (gi >= 0 && gd < INFINITY) { kd = gd; ki = gi; }
  }
  int rank = 0;
#pragma unroll
  for (int e = 0; e < 2 * PKMAX; ++e) {
    const float od = __shfl(kd, e, 64);
    const long long oi = __shfl(ki, e, 64);
    rank += (od < kd || (od == kd && (oi < ki || (oi == ki && e < lane)))) ? 1 : 0;
  }
  if (lane < 2 * PKMAX && rank < p.k) {
    const bool qok = finite_f(p.qn[qrow]);
    p.idx[qrow * p.k + rank] = (qok && kd < INFINITY) ? ki : -1;
    p.d2[qrow * p.k + rank] = qok ? kd : qnan_f();
  }
}

// reference tiles per workgroup of the candidate walk: as many strips as bring the grid to KNN_WGS workgroups, at most one per tile
int knn_strip_of(int M, int N) {
  const long long want = (KNN_WGS + tiles_of(M) - 1) / tiles_of(M);
  return (int)std::max<long long>(1, tiles_of(N) / want);
}
long long knn_strips_of(int M, int N) { const int s = knn_strip_of(M, N); return (tiles_of(N) + s - 1) / s; }

}  // namespace

extern "C" size_t jck_knn_index_ws_bytes(int M, int N) {
  if (M < 1 || N < 1 || M > P_MAX_ROWS || N > P_MAX_ROWS) return 0;
  return (size_t)M * (size_t)(1 + 2 * PKMAX * knn_strips_of(M, N)) * sizeof(float);
}

extern "C" int jck_knn_index_f32(const float* q, int M, const float* ref, int N, int D, int k, long long q_base, long long ref_base,
                                 int exclude_self, int merge, long long* idx, float* d2, void* ws, void* stream) {
  if (!q || !ref || !idx || !d2 || !ws || M < 1 || N < 1 || D < 1 || M > P_MAX_ROWS || N > P_MAX_ROWS) JCK_FAIL(JCK_E_ARG, "knn_index: bad arguments");
  if (k < 1 || k > PKMAX) JCK_FAIL(JCK_E_ARG, "knn_index: k must be 1..8");
  const long long strips = knn_strips_of(M, N);
  float* qn = (float*)ws;
  float* cd = qn + M;
  int* ci = (int*)(cd + (long long)M * strips * PKMAX);
  KnnCandP c = {};
  c.q = q; c.ref = ref; c.M = M; c.N = N; c.D = D; c.vec = vec_ok(q, ref, D); c.strip = knn_strip_of(M, N); c.nstrips = (int)strips;
  c.exclude = exclude_self != 0; c.self_off = q_base - ref_base; c.qn = qn; c.cd = cd; c.ci = ci;
  hipLaunchKernelGGL(knn_cand_kernel, dim3((unsigned)tiles_of(M), (unsigned)strips), dim3(256), 0, (hipStream_t)stream, c);
  HIPCHK(hipGetLastError());
  KnnRankP r = {};
  r.q = q; r.ref = ref; r.M = M; r.D = D; r.vec = c.vec; r.k = k; r.nstrips = (int)strips; r.merge = merge != 0; r.ref_base = ref_base;
  r.qn = qn; r.cd = cd; r.ci = ci; r.idx = idx; r.d2 = d2;
  hipLaunchKernelGGL(knn_rank_kernel, dim3((unsigned)(((long long)M + 3) / 4)), dim3(256), 0, (hipStream_t)stream, r);
  HIPCHK(hipGetLastError());
  return JCK_OK;
}
