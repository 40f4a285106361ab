// Pairwise statistics over feature matrices for the evaluation branch: KID (the unbiased MMD^2 with the cubic polynomial
// kernel) and improved precision / recall (k-NN manifolds in feature space).  The large side is the cached real features
// (50 000 x 100 for CIFAR-100): real x real is 2.5e9 pairs, so nothing here ever writes an M x N matrix.
//
//   jck_poly3_sum_f64     out[0] = sum_{i,j} (gamma * <x_i, y_j> + coef0)^3, optionally without the pairs i == j
//   jck_knn_radius2_f32   r2[i]  = k-th smallest squared distance from x_i to the other rows of x
//   jck_manifold_hit_u8   hit[i] = 1 when q_i lies inside the k-NN ball of some reference row
//   jck_pairstat_ws_bytes workspace of the first (host only)
//
// The three are epilogues of one Gram-tile walk (pairtile.hpp: the tile, its staging, the norms and the k-smallest list; the nearest
// rows WITH their indices, jck_knn_index_f32, live in knnindex.hip over the same core).  A workgroup owns one 64-row block of `b`
// and walks 64-row tiles of `a`; d^2 = max(0, (|a|^2 + |b|^2) - 2 G) in fp32, in that association.
//
// Determinism: no float atomics.  The polynomial sum is fp64 per lane in a fixed order, wave and workgroup sums in
// a fixed order, one partial per workgroup into the caller's workspace, and a second one-workgroup launch adds the partials
// in a fixed order.  Non-finite values: the sums carry them; a row with a non-finite norm gets radius NaN / hit 255, and a
// NaN distance or radius compares false, so such a reference row is never a neighbour and never hit.
#include "pairtile.hpp"

namespace {

constexpr int PSTRIP = 8;
enum { EPI_POLY3 = 0, EPI_KNN = 1, EPI_HIT = 2 };

struct PairP {
  const float* a; const float* b;      // a: the walked rows (tile rows); b: the workgroup's own block (tile columns)
  int Ma, Nb, D, vec, strip, skip_diag, k;
  double gamma, coef0;
  double* ws; float* r2out; const float* r2in; unsigned char* hit;
};

template <int EPI>
__global__ __launch_bounds__(256) void pair_kernel(const PairP p) {
  __shared__ __attribute__((aligned(16))) float As[PT][PLD];
  __shared__ __attribute__((aligned(16))) float Bs[PT][PLD];
  __shared__ float nA[PT], nB[PT], r2s[PT];
  __shared__ int hitf[PT];
  __shared__ float cand[EPI == EPI_KNN ? PT * 8 * PKMAX : 1];
  __shared__ double wsum[4];
  const TilePos t(threadIdx.x);
  const int tid = t.tid, lane = t.lane, wave = t.wave;
  const int b0 = (int)blockIdx.x * PT;
  const long long tilesA = ((long long)p.Ma + PT - 1) / PT;
  const long long t0 = (long long)blockIdx.y * p.strip, t1 = t0 + p.strip < tilesA ? t0 + p.strip : tilesA;
  double psum = 0.0;
  TopK<false> L[2];
  bool h[2] = {false, false};
#pragma unroll
  for (int j = 0; j < 2; ++j) L[j].clear();
  if (EPI == EPI_HIT && tid < PT) hitf[tid] = 0;

  for (long long ta = t0; ta < t1; ++ta) {
    const int a0 = (int)(ta * PT);
    f32x4 acc[2][2];
    gram_tile<1, EPI != EPI_POLY3>(acc, &As, &Bs, nA, nB, p.a, p.Ma, a0, p.b, p.Nb, b0, p.D, p.vec, ta == t0, t);
    if (EPI != EPI_POLY3) {
      if (EPI == EPI_HIT && wave == 2) r2s[lane] = (a0 + lane < p.Ma) ? p.r2in[a0 + lane] : qnan_f();
      __syncthreads();
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int cb = t.col(j), gb = b0 + cb;
      const float nb = EPI != EPI_POLY3 ? nB[cb] : 0.f;
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int ra = t.row(i, r), ga = a0 + ra;
          const float g = acc[i][j][r];
          if (EPI == EPI_POLY3) {
            if (ga < p.Ma && gb < p.Nb && !(p.skip_diag && ga == gb)) {
              const double v = fma(p.gamma, (double)g, p.coef0);
              psum += v * v * v;
            }
          } else {
            float d = (nA[ra] + nb) - 2.f * g;
            d = d < 0.f ? 0.f : d;                                      // NaN stays NaN
            if (EPI == EPI_KNN) {
              if (ga < p.Ma && ga != gb) L[j].offer(d);
            } else {
              h[j] = h[j] || (d <= r2s[ra]);                            // rows past Ma carry a NaN radius
            }
          }
        }
    }
    if (EPI == EPI_HIT) {                                               // leave the walk once every row of the block is decided
#pragma unroll
      for (int j = 0; j < 2; ++j)
        if (h[j]) hitf[t.col(j)] = 1;
      __syncthreads();
      const int decided = hitf[lane] | (b0 + lane >= p.Nb) | !finite_f(nB[lane]);
      if (__syncthreads_and(decided)) break;
    }
  }

  if (EPI == EPI_POLY3) {
    psum = wave_sum_d(psum);
    if (lane == 0) wsum[wave] = psum;
    __syncthreads();
    if (tid == 0) p.ws[(long long)blockIdx.y * gridDim.x + blockIdx.x] = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
  } else if (EPI == EPI_KNN) {
    TopK<false> M;
    merge_columns(M, L, cand, nullptr, t);
    if (tid < PT && b0 + tid < p.Nb) {
      float res = M.v[0];
#pragma unroll
      for (int e = 1; e < PKMAX; ++e) res = (e == p.k - 1) ? M.v[e] : res;
      p.r2out[b0 + tid] = finite_f(nB[tid]) ? res : qnan_f();
    }
  } else {
    if (tid < PT && b0 + tid < p.Nb) p.hit[b0 + tid] = finite_f(nB[tid]) ? (unsigned char)(hitf[tid] != 0) : (unsigned char)255;
  }
}

// out[0] = sum of n partials: one workgroup, fixed order
__global__ __launch_bounds__(256) void sum_partials_f64_kernel(const double* __restrict__ ws, long long n, double* __restrict__ out) {
  __shared__ double sm[256];
  double s = 0.0;
  for (long long i = threadIdx.x; i < n; i += 256) s += ws[i];
  sm[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) sm[threadIdx.x] += sm[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = sm[0];
}

// walked tiles per workgroup of the polynomial sum: PSTRIP, more only where the grid's y extent would overflow
int strip_of(int M) { return (int)std::max<long long>(PSTRIP, (tiles_of(M) + 32767) / 32768); }
long long strips_of(int M) { const int s = strip_of(M); return (tiles_of(M) + s - 1) / s; }

}  // namespace

extern "C" size_t jck_pairstat_ws_bytes(int M, int N) {
  if (M < 1 || N < 1 || M > P_MAX_ROWS || N > P_MAX_ROWS) return 0;
  return (size_t)(tiles_of(N) * strips_of(M)) * sizeof(double);
}

extern "C" int jck_poly3_sum_f64(const float* x, int M, const float* y, int N, int D, double gamma, double coef0, int skip_diag,
                                 double* out, double* ws, void* stream) {
  if (!x || !y || !out || !ws || M < 1 || N < 1 || D < 1 || M > P_MAX_ROWS || N > P_MAX_ROWS) JCK_FAIL(JCK_E_ARG, "poly3_sum: bad arguments");
  PairP p = {};
  p.a = x; p.Ma = M; p.b = y; p.Nb = N; p.D = D; p.vec = vec_ok(x, y, D); p.strip = strip_of(M); p.skip_diag = skip_diag != 0;
  p.gamma = gamma; p.coef0 = coef0; p.ws = ws;
  const long long gx = tiles_of(N), gy = strips_of(M);
  hipLaunchKernelGGL(pair_kernel<EPI_POLY3>, dim3((unsigned)gx, (unsigned)gy), dim3(256), 0, (hipStream_t)stream, p);
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(sum_partials_f64_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const double*)ws, gx * gy, out);
  HIPCHK(hipGetLastError());
  return JCK_OK;
}

extern "C" int jck_knn_radius2_f32(const float* x, int N, int D, int k, float* r2, void* stream) {
  if (!x || !r2 || N < 1 || D < 1 || N > P_MAX_ROWS) JCK_FAIL(JCK_E_ARG, "knn_radius2: bad arguments");
  if (k < 1 || k > PKMAX) JCK_FAIL(JCK_E_ARG, "knn_radius2: k must be 1..8");
  if (k >= N) JCK_FAIL(JCK_E_ARG, "knn_radius2: k must be smaller than the number of rows");
  PairP p = {};
  p.a = x; p.Ma = N; p.b = x; p.Nb = N; p.D = D; p.vec = vec_ok(x, x, D); p.strip = (int)tiles_of(N); p.k = k; p.r2out = r2;
  hipLaunchKernelGGL(pair_kernel<EPI_KNN>, dim3((unsigned)tiles_of(N)), dim3(256), 0, (hipStream_t)stream, p);
  HIPCHK(hipGetLastError());
  return JCK_OK;
}

extern "C" int jck_manifold_hit_u8(const float* q, int M, const float* ref, const float* r2, int N, int D, unsigned char* hit,
                                   void* stream) {
  if (!q || !ref || !r2 || !hit || M < 1 || N < 1 || D < 1 || M > P_MAX_ROWS || N > P_MAX_ROWS) JCK_FAIL(JCK_E_ARG, "manifold_hit: bad arguments");
  PairP p = {};
  p.a = ref; p.Ma = N; p.b = q; p.Nb = M; p.D = D; p.vec = vec_ok(q, ref, D); p.strip = (int)tiles_of(N); p.r2in = r2; p.hit = hit;
  hipLaunchKernelGGL(pair_kernel<EPI_HIT>, dim3((unsigned)tiles_of(M)), dim3(256), 0, (hipStream_t)stream, p);
  HIPCHK(hipGetLastError());
  return JCK_OK;
}
