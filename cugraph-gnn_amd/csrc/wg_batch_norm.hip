// Training-mode batch normalisation over the rows of a layer (torch.nn.BatchNorm1d between the two Linears of PyG's MLP; the
// GIN route "mlp_bn" of wholegraph_amd.nn.GINConv), split where the statistics force it:
//     z [n, H]  --partials-->  (mean, M2, count) per 16-row tile  --finalize-->  mean, rstd, scale = gamma rstd, shift = beta - mean scale
//     out = act(relu(z scale + shift) @ W2^T + b2)                                                        (the tail, one launch)
// and the backward of the normalisation with the ReLU behind it:
//     dy = dHidden [hidden > 0],  x^ = (z - mean) rstd,  dbeta = sum dy,  dgamma = sum dy x^,
//     dz = gamma rstd (dy - dbeta / n - x^ dgamma / n)
//
// Pieces:
//   * bn_partials_kernel — the (mean, M2) of every column over each 16-row tile, two passes inside the tile (column_mean_m2,
//     wg_layer_parts.hpp); the GIN layer kernel's STATS variant (wg_gin.hip) writes the same records from its LDS tile.
//   * bn_finalize_kernel — one workgroup of 1024 threads per float4 of columns.  Thread c combines the tiles of chunk c (a
//     contiguous run of ceil(T / 1024) tiles, in tile order) with Chan, Golub and LeVeque's pairwise update of (count, mean, M2)
//     ("Updating formulae and a pairwise algorithm for computing sample variances", 1979); the 1024 chunk records are then
//     combined by a fixed halving tree in LDS.  No atomics, no sum of squares; the order depends on T alone.
//   * bn_act_linear_kernel — 16-row tiles: relu(z scale + shift) -> LDS tile (and hidden_out), then tile_times_wt with W2.
//   * bn_bwd_reduce_kernel / bn_bwd_combine_kernel — per-workgroup partial rows of (sum dy x^, sum dy), row groups added in group
//     order through LDS, then the partial rows added in a fixed order (the pattern of wg_norm_act.hip's affine gradients).
//   * bn_bwd_apply_kernel — dz, one pass.
#include "wg_layer_parts.hpp"

namespace wgamd {
namespace {

constexpr int kFinThreads = 1024;     // chunks per column group of the finalize launch
constexpr int kBwdBlocks = 1024;      // partial rows of the backward reduction at most
constexpr int kCombCols = 64, kCombLanes = 16;

__global__ void __launch_bounds__(kThreads) bn_partials_kernel(const float* z, int64_t ldz, int64_t n_rows, int H, float* partials,
                                                               int* counts, int64_t tile0)
{
  const int64_t row0 = (int64_t)blockIdx.x * kTileRows;
  const int rows_here = (int)std::min<int64_t>(kTileRows, n_rows - row0);
  const int64_t t = tile0 + blockIdx.x;
  for (int c = threadIdx.x; c < H; c += kThreads) {
    float mean, m2;
    column_mean_m2(z + row0 * ldz + c, ldz, rows_here, mean, m2);
    partials[t * 2 * H + c] = mean;
    partials[(t * 2 + 1) * H + c] = m2;
  }
  if (threadIdx.x == 0) counts[t] = rows_here;
}

// (na, ma, Ma) <- the record of the union of a and b
__device__ __forceinline__ void chan_combine(float& na, f32x4& ma, f32x4& Ma, float nb, const f32x4& mb, const f32x4& Mb)
{
  if (nb == 0.f) return;
  if (na == 0.f) {
    na = nb, ma = mb, Ma = Mb;
    return;
  }
  const float n = na + nb, w = nb / n;
  const f32x4 d = mb - ma;
  ma += d * w;
  Ma += Mb + d * d * (na * w);
  na = n;
}

struct fin_args {
  const float* partials;
  const int* counts;
  int64_t T;
  int H;
  const float* gamma;
  const float* beta;
  float eps, momentum;
  float* running_mean;
  float* running_var;
  float* mean;
  float* var;
  float* rstd;
  float* scale;
  float* shift;
};

__global__ void __launch_bounds__(kFinThreads) bn_finalize_kernel(fin_args a)
{
  __shared__ float cnt[kFinThreads];
  __shared__ f32x4 mu[kFinThreads], m2[kFinThreads];
  const int c = threadIdx.x, q = blockIdx.x;      // chunk, float4 of columns
  const int64_t per = (a.T + kFinThreads - 1) / kFinThreads;
  const int64_t t0 = std::min<int64_t>(a.T, c * per), t1 = std::min<int64_t>(a.T, t0 + per);
  float n = 0.f;
  f32x4 m = {0.f, 0.f, 0.f, 0.f}, M = {0.f, 0.f, 0.f, 0.f};
  for (int64_t t = t0; t < t1; ++t) {
    const f32x4* rec = reinterpret_cast<const f32x4*>(a.partials + t * 2 * a.H);
    chan_combine(n, m, M, (float)a.counts[t], rec[q], rec[a.H / 4 + q]);
  }
  cnt[c] = n, mu[c] = m, m2[c] = M;
  __syncthreads();
  for (int s = kFinThreads / 2; s >= 1; s >>= 1) {
    if (c < s) {
      chan_combine(n, m, M, cnt[c + s], mu[c + s], m2[c + s]);
      cnt[c] = n, mu[c] = m, m2[c] = M;
    }
    __syncthreads();
  }
  if (c >= 4) return;
  n = cnt[0];
  const int col = 4 * q + c;
  const float mean = mu[0][c], var = n > 0.f ? m2[0][c] / n : 0.f;
  const float rstd = 1.f / sqrtf(var + a.eps);
  const float scale = (a.gamma ? a.gamma[col] : 1.f) * rstd;
  a.mean[col] = mean;
  if (a.var) a.var[col] = var;
  if (a.rstd) a.rstd[col] = rstd;
  if (a.scale) a.scale[col] = scale;
  if (a.shift) a.shift[col] = (a.beta ? a.beta[col] : 0.f) - mean * scale;
  if (a.running_mean) a.running_mean[col] = (1.f - a.momentum) * a.running_mean[col] + a.momentum * mean;
  if (a.running_var) {
    const float unbiased = n > 1.f ? m2[0][c] / (n - 1.f) : var;
    a.running_var[col] = (1.f - a.momentum) * a.running_var[col] + a.momentum * unbiased;
  }
}

struct tail_args {
  const float* z;
  int64_t ldz, n_rows;
  int H, H16, SH;
  const float* scale;
  const float* shift;
  const float* w2;
  int64_t ldw2;
  int N;
  const float* b2;
  int relu_out;
  float* out;
  int64_t ldo;
  float* hidden_out;
  int64_t ld_hidden;
};

__global__ void __launch_bounds__(kThreads) bn_act_linear_kernel(tail_args a)
{
  extern __shared__ __attribute__((aligned(16))) float hid[];
  const int64_t row0 = (int64_t)blockIdx.x * kTileRows;
  const int H4 = a.H / 4, H16q = a.H16 / 4;
  for (int p = threadIdx.x; p < kTileRows * H16q; p += kThreads) {
    const int r = p / H16q, q = p % H16q;
    f32x4 h = {0.f, 0.f, 0.f, 0.f};
    if (q < H4 && row0 + r < a.n_rows) {
      const f32x4 zv = reinterpret_cast<const f32x4*>(a.z + (row0 + r) * a.ldz)[q];
      const f32x4 sc = reinterpret_cast<const f32x4*>(a.scale)[q], sh = reinterpret_cast<const f32x4*>(a.shift)[q];
#pragma unroll
      for (int e = 0; e < 4; ++e) h[e] = fmaxf(__builtin_fmaf(zv[e], sc[e], sh[e]), 0.f);
      if (a.hidden_out) reinterpret_cast<f32x4*>(a.hidden_out + (row0 + r) * a.ld_hidden)[q] = h;
    }
    reinterpret_cast<f32x4*>(hid + r * a.SH)[q] = h;
  }
  __syncthreads();
  tile_times_wt(hid, a.SH, a.H, a.H16, a.w2, a.ldw2, a.N, a.b2, a.relu_out, a.out, a.ldo, row0, a.n_rows);
}

struct bwd_args {
  const float* dh;
  int64_t ld_dh;
  const float* hidden;
  int64_t ld_hidden;
  const float* z;
  int64_t ldz, n_rows;
  int H, blocks;
  const float* mean;
  const float* rstd;
  const float* gamma;
  float* part;          // [blocks][2][H]: sum dy x^, sum dy
  float* dgamma;
  float* dbeta;
  float* dz;
  int64_t ld_dz;
};

inline int lanes_of(int H)      // lanes that hold a row, one float4 each: 4 .. 64
{
  int lg = 4;
  while (lg < H / 4) lg *= 2;
  return lg;
}

// dy = dHidden [hidden > 0] and x^ of float4 q of row r
__device__ __forceinline__ void dy_xhat(const bwd_args& a, int64_t r, int q, const f32x4& mean, const f32x4& rstd, f32x4& dy, f32x4& xh)
{
  const f32x4 g = reinterpret_cast<const f32x4*>(a.dh + r * a.ld_dh)[q];
  const f32x4 h = reinterpret_cast<const f32x4*>(a.hidden + r * a.ld_hidden)[q];
  const f32x4 zv = reinterpret_cast<const f32x4*>(a.z + r * a.ldz)[q];
#pragma unroll
  for (int e = 0; e < 4; ++e) dy[e] = h[e] > 0.f ? g[e] : 0.f;
  xh = (zv - mean) * rstd;
}

template <int LG>
__global__ void __launch_bounds__(kThreads) bn_bwd_reduce_kernel(bwd_args a)
{
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int RP = kThreads / LG;
  const int grp = threadIdx.x / LG, q = threadIdx.x % LG, H4 = a.H / 4;
  const bool col_ok = q < H4;
  const int64_t tiles = (a.n_rows + RP - 1) / RP;
  f32x4 mean = {0.f, 0.f, 0.f, 0.f}, rstd = mean, s1 = mean, s2 = mean;
  if (col_ok) mean = reinterpret_cast<const f32x4*>(a.mean)[q], rstd = reinterpret_cast<const f32x4*>(a.rstd)[q];
  for (int64_t t = blockIdx.x; t < tiles; t += a.blocks) {
    const int64_t r = t * RP + grp;
    if (col_ok && r < a.n_rows) {
      f32x4 dy, xh;
      dy_xhat(a, r, q, mean, rstd, dy, xh);
      s1 += dy * xh, s2 += dy;
    }
  }
  const int C2 = 2 * a.H;
  if (col_ok) {
    reinterpret_cast<f32x4*>(lds + grp * C2)[q] = s1;
    reinterpret_cast<f32x4*>(lds + grp * C2 + a.H)[q] = s2;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < C2; i += kThreads) {
    float acc = 0.f;
    for (int g = 0; g < RP; ++g) acc += lds[g * C2 + i];
    a.part[(int64_t)blockIdx.x * C2 + i] = acc;
  }
}

// dgamma[c] = sum over the partial rows of part[b][0][c], dbeta[c] = ... part[b][1][c]: lane l of 16 adds rows l, l + 16, ... in
// order, then the 16 lane sums are added in lane order.  grid ceil(2 H / 64)
__global__ void __launch_bounds__(kCombCols* kCombLanes) bn_bwd_combine_kernel(bwd_args a)
{
  __shared__ float t[kCombLanes][kCombCols];
  const int C2 = 2 * a.H, col = threadIdx.x % kCombCols, l = threadIdx.x / kCombCols;
  const int i = blockIdx.x * kCombCols + col;
  float acc = 0.f;
  if (i < C2)
    for (int b = l; b < a.blocks; b += kCombLanes) acc += a.part[(int64_t)b * C2 + i];
  t[l][col] = acc;
  __syncthreads();
  if (l != 0 || i >= C2) return;
  acc = 0.f;
  for (int k = 0; k < kCombLanes; ++k) acc += t[k][col];
  if (i < a.H) a.dgamma[i] = acc;
  else a.dbeta[i - a.H] = acc;
}

__global__ void __launch_bounds__(kThreads) bn_bwd_apply_kernel(bwd_args a)
{
  const int H4 = a.H / 4;
  const int64_t total = a.n_rows * H4;
  const float inv_n = 1.f / (float)a.n_rows;
  for (int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x; p < total; p += (int64_t)gridDim.x * kThreads) {
    const int64_t r = p / H4;
    const int q = (int)(p % H4);
    const f32x4 mean = reinterpret_cast<const f32x4*>(a.mean)[q], rstd = reinterpret_cast<const f32x4*>(a.rstd)[q];
    f32x4 gam = {1.f, 1.f, 1.f, 1.f};
    if (a.gamma) gam = reinterpret_cast<const f32x4*>(a.gamma)[q];
    const f32x4 dg = reinterpret_cast<const f32x4*>(a.dgamma)[q], db = reinterpret_cast<const f32x4*>(a.dbeta)[q];
    f32x4 dy, xh;
    dy_xhat(a, r, q, mean, rstd, dy, xh);
    reinterpret_cast<f32x4*>(a.dz + r * a.ld_dz)[q] = gam * rstd * (dy - db * inv_n - xh * (dg * inv_n));
  }
}

inline bool vec_ok(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

void require_width(int H)
{
  if (!wgamd_batch_norm_supported(H)) throw logic_error(fmt("unsupported width H=%d (multiple of 4, 4 .. 256)", H));
}

// the operands the two backward entries share, checked
bwd_args make_bwd_args(const float* dh, int64_t ld_dh, const float* hidden, int64_t ld_hidden, const float* z, int64_t ldz,
                       int64_t n_rows, int H, const float* mean, const float* rstd)
{
  WG_REQUIRE_INPUT(n_rows >= 0, "bad sizes");
  require_width(H);
  bwd_args a{};
  if (n_rows == 0) return a;
  WG_REQUIRE_INPUT(dh && hidden && z && mean && rstd, "null pointer");
  WG_REQUIRE_INPUT(ld_dh >= H && ld_hidden >= H && ldz >= H, "leading dimension too small");
  if (!aligned_rows(dh, ld_dh) || !aligned_rows(hidden, ld_hidden) || !aligned_rows(z, ldz) || !vec_ok(mean) || !vec_ok(rstd))
    throw logic_error("dhidden / hidden / z rows, mean and rstd must be 16-B aligned");
  a.dh = dh, a.ld_dh = ld_dh, a.hidden = hidden, a.ld_hidden = ld_hidden, a.z = z, a.ldz = ldz, a.n_rows = n_rows, a.H = H;
  a.mean = mean, a.rstd = rstd;
  return a;
}

}  // namespace
}  // namespace wgamd

extern "C" int wgamd_batch_norm_supported(int H) { return H % 4 == 0 && H >= 4 && H <= 256; }

extern "C" int64_t wgamd_bn_bwd_blocks(int64_t n_rows, int H)
{
  if (n_rows <= 0 || !wgamd_batch_norm_supported(H)) return 0;
  const int rp = wgamd::kThreads / wgamd::lanes_of(H);
  return std::min<int64_t>((n_rows + rp - 1) / rp, wgamd::kBwdBlocks);
}

extern "C" wholememory_error_code_t wgamd_bn_partials_f32(const float* z, int64_t ldz, int64_t n_rows, int H, float* partials,
                                                          int* counts, int64_t tile0, void* stream)
{
  using namespace wgamd;
  return guarded("wgamd_bn_partials_f32", [&] {
    WG_REQUIRE_INPUT(n_rows >= 0 && tile0 >= 0, "bad sizes");
    require_width(H);
    if (n_rows == 0) return;
    WG_REQUIRE_INPUT(z && partials && counts, "null pointer");
    WG_REQUIRE_INPUT(ldz >= H, "leading dimension too small");
    if (!aligned_rows(z, ldz) || !vec_ok(partials)) throw logic_error("z rows and partials must be 16-B aligned");
    const unsigned tiles = (unsigned)((n_rows + kTileRows - 1) / kTileRows);
    bn_partials_kernel<<<tiles, kThreads, 0, static_cast<hipStream_t>(stream)>>>(z, ldz, n_rows, H, partials, counts, tile0);
    WG_HIP_CHECK(hipGetLastError());
  });
}

extern "C" wholememory_error_code_t wgamd_bn_finalize_f32(const float* partials, const int* counts, int64_t n_tiles, int H,
                                                          const float* gamma, const float* beta, float eps, float momentum,
                                                          float* running_mean, float* running_var, float* mean, float* var,
                                                          float* rstd, float* scale, float* shift, void* stream)
{
  using namespace wgamd;
  return guarded("wgamd_bn_finalize_f32", [&] {
    WG_REQUIRE_INPUT(n_tiles >= 0 && eps >= 0.f, "bad sizes");
    require_width(H);
    WG_REQUIRE_INPUT(mean && (n_tiles == 0 || (partials && counts)), "null pointer");
    if (!vec_ok(partials)) throw logic_error("partials must be 16-B aligned");
    fin_args a{partials, counts, n_tiles, H, gamma, beta, eps, momentum, running_mean, running_var, mean, var, rstd, scale, shift};
    bn_finalize_kernel<<<(unsigned)(H / 4), kFinThreads, 0, static_cast<hipStream_t>(stream)>>>(a);
    WG_HIP_CHECK(hipGetLastError());
  });
}

extern "C" wholememory_error_code_t wgamd_bn_act_linear_f32(const float* z, int64_t ldz, int64_t n_rows, int H, const float* scale,
                                                            const float* shift, const float* w2, int64_t ldw2, int N,
                                                            const float* b2, int relu_out, float* out, int64_t ldo,
                                                            float* hidden_out, int64_t ld_hidden, void* stream)
{
  using namespace wgamd;
  return guarded("wgamd_bn_act_linear_f32", [&] {
    WG_REQUIRE_INPUT(n_rows >= 0, "bad sizes");
    require_width(H);
    if (!(N > 0 && N <= 256)) throw logic_error(fmt("unsupported width N=%d (1 .. 256)", N));
    if (n_rows == 0) return;
    WG_REQUIRE_INPUT(z && scale && shift && w2 && out, "null pointer");
    WG_REQUIRE_INPUT(ldz >= H && ldw2 >= H && ldo >= N && (hidden_out == nullptr || ld_hidden >= H), "leading dimension too small");
    if (!aligned_rows(z, ldz) || !aligned_rows(w2, ldw2) || (hidden_out && !aligned_rows(hidden_out, ld_hidden)) || !vec_ok(scale) ||
        !vec_ok(shift))
      throw logic_error("z / w2 / hidden_out rows, scale and shift must be 16-B aligned");
    tail_args a{};
    a.z = z, a.ldz = ldz, a.n_rows = n_rows, a.H = H, a.H16 = (H + 15) / 16 * 16, a.SH = a.H16 + 4;
    a.scale = scale, a.shift = shift, a.w2 = w2, a.ldw2 = ldw2, a.N = N, a.b2 = b2, a.relu_out = relu_out != 0;
    a.out = out, a.ldo = ldo, a.hidden_out = hidden_out, a.ld_hidden = ld_hidden;
    const unsigned tiles = (unsigned)((n_rows + kTileRows - 1) / kTileRows);
    const size_t lds = (size_t)kTileRows * a.SH * 4;      // at most 16 x 260 floats = 16.6 KB
    bn_act_linear_kernel<<<tiles, kThreads, lds, static_cast<hipStream_t>(stream)>>>(a);
    WG_HIP_CHECK(hipGetLastError());
  });
}

extern "C" wholememory_error_code_t wgamd_bn_bwd_reduce_f32(const float* dhidden, int64_t ld_dh, const float* hidden,
                                                            int64_t ld_hidden, const float* z, int64_t ldz, int64_t n_rows, int H,
                                                            const float* mean, const float* rstd, float* partials, float* dgamma,
                                                            float* dbeta, void* stream)
{
  using namespace wgamd;
  return guarded("wgamd_bn_bwd_reduce_f32", [&] {
    bwd_args a = make_bwd_args(dhidden, ld_dh, hidden, ld_hidden, z, ldz, n_rows, H, mean, rstd);
    WG_REQUIRE_INPUT(dgamma && dbeta && (n_rows == 0 || partials), "null pointer");
    a.H = H, a.part = partials, a.dgamma = dgamma, a.dbeta = dbeta;
    a.blocks = (int)wgamd_bn_bwd_blocks(n_rows, H);      // no rows: no partial rows, zeros
    auto st = static_cast<hipStream_t>(stream);
    if (a.blocks > 0) {
      const int lg = lanes_of(H);
      const size_t lds = (size_t)(kThreads / lg) * 2 * H * sizeof(float);      // 8 KB at most
      switch (lg) {
        case 4: bn_bwd_reduce_kernel<4><<<a.blocks, kThreads, lds, st>>>(a); break;
        case 8: bn_bwd_reduce_kernel<8><<<a.blocks, kThreads, lds, st>>>(a); break;
        case 16: bn_bwd_reduce_kernel<16><<<a.blocks, kThreads, lds, st>>>(a); break;
        case 32: bn_bwd_reduce_kernel<32><<<a.blocks, kThreads, lds, st>>>(a); break;
        default: bn_bwd_reduce_kernel<64><<<a.blocks, kThreads, lds, st>>>(a); break;
      }
      WG_HIP_CHECK(hipGetLastError());
    }
    bn_bwd_combine_kernel<<<(unsigned)((2 * H + kCombCols - 1) / kCombCols), kCombCols * kCombLanes, 0, st>>>(a);
    WG_HIP_CHECK(hipGetLastError());
  });
}

extern "C" wholememory_error_code_t wgamd_bn_bwd_apply_f32(const float* dhidden, int64_t ld_dh, const float* hidden,
                                                           int64_t ld_hidden, const float* z, int64_t ldz, int64_t n_rows, int H,
                                                           const float* mean, const float* rstd, const float* gamma,
                                                           const float* dgamma, const float* dbeta, float* dz, int64_t ld_dz,
                                                           void* stream)
{
  using namespace wgamd;
  return guarded("wgamd_bn_bwd_apply_f32", [&] {
    bwd_args a = make_bwd_args(dhidden, ld_dh, hidden, ld_hidden, z, ldz, n_rows, H, mean, rstd);
    if (n_rows == 0) return;
    WG_REQUIRE_INPUT(dgamma && dbeta && dz, "null pointer");
    WG_REQUIRE_INPUT(ld_dz >= H, "leading dimension too small");
    if (!aligned_rows(dz, ld_dz) || !vec_ok(gamma) || !vec_ok(dgamma) || !vec_ok(dbeta))
      throw logic_error("dz rows, gamma, dgamma and dbeta must be 16-B aligned");
    a.gamma = gamma, a.dgamma = const_cast<float*>(dgamma), a.dbeta = const_cast<float*>(dbeta), a.dz = dz, a.ld_dz = ld_dz;
    const int64_t total = n_rows * (H / 4);
    const unsigned blocks = (unsigned)std::min<int64_t>((total + kThreads - 1) / kThreads, 8192);
    bn_bwd_apply_kernel<<<blocks, kThreads, 0, static_cast<hipStream_t>(stream)>>>(a);
    WG_HIP_CHECK(hipGetLastError());
  });
}
