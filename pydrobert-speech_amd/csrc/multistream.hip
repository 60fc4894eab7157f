// Batched streaming (multistream.py::StreamBatch): one tick's packed work buffer from the carried samples of many
// streams and their new chunks, and the new carries, in one launch.
//
// Every stream of the tick is one entry of `meta` (int64[n][MS_FIELDS], fields below).  Its work span is
//   work[work_off + j] = j < carry_len ? pool[half][stream][j] : chunks[chunk_off + drop + j - carry_len]
// for j < avail = carry_len + chunk_len - drop, and its new carry is work[new_carry .. avail), written to the OTHER
// half of the pool (ping-pong: a tick reads one half of a stream's slot and writes the other, so no block reads what
// another block of the same stream writes).  The STFT batch launches then read the work buffer with explicit
// per-stream frame counts.  Work is dealt in tiles of MS_TILE samples of one stream; `tile_prefix[e]` is the first
// tile of entry e, so one long chunk spreads over many workgroups and a tick of short ones takes one each.
#include "pds_internal.h"

namespace pds {

enum { MS_STREAM = 0, MS_CHUNK_OFF, MS_CHUNK_LEN, MS_CARRY_LEN, MS_DROP, MS_NEW_CARRY, MS_WORK_OFF, MS_HALF, MS_FIELDS };
constexpr int MS_THREADS = 256;
constexpr int MS_PER_THREAD = 4;
constexpr int64_t MS_TILE = MS_THREADS * MS_PER_THREAD;

static int32_t invalid_ms(const char *msg) {
  set_error(msg);
  return PDS_ERR_INVALID;
}

template <typename T>
__global__ __launch_bounds__(MS_THREADS) void multistream_assemble_kernel(
    const T *__restrict__ chunks, T *__restrict__ pool, int64_t capacity, int32_t L,
    const int64_t *__restrict__ meta, const int64_t *__restrict__ tile_prefix, int32_t n, T *__restrict__ work) {
  const int64_t tile = blockIdx.x;
  // entry of this tile: the last e with tile_prefix[e] <= tile (entries without samples have no tile)
  int lo = 0, hi = n;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (tile_prefix[mid] <= tile) lo = mid; else hi = mid;
  }
  const int64_t *m = meta + (int64_t)lo * MS_FIELDS;
  const int64_t s = m[MS_STREAM], carry_len = m[MS_CARRY_LEN], new_carry = m[MS_NEW_CARRY];
  const int64_t avail = carry_len + m[MS_CHUNK_LEN] - m[MS_DROP];
  const int64_t chunk_at = m[MS_CHUNK_OFF] + m[MS_DROP] - carry_len;  // chunks[chunk_at + j] is work sample j >= carry_len
  const int64_t half = m[MS_HALF] & 1;
  const T *carry_in = pool + (half * capacity + s) * (int64_t)L;
  T *carry_out = pool + ((1 - half) * capacity + s) * (int64_t)L;
  T *dst = work + m[MS_WORK_OFF];
  const int64_t j0 = (tile - tile_prefix[lo]) * MS_TILE;
  const int64_t j1 = j0 + MS_TILE < avail ? j0 + MS_TILE : avail;
  // loads of the tile first, then the stores (four independent loads in flight per lane)
  T v[MS_PER_THREAD];
#pragma unroll
  for (int q = 0; q < MS_PER_THREAD; ++q) {
    const int64_t j = j0 + q * MS_THREADS + threadIdx.x;
    v[q] = j < j1 ? (j < carry_len ? carry_in[j] : chunks[chunk_at + j]) : T(0);
  }
#pragma unroll
  for (int q = 0; q < MS_PER_THREAD; ++q) {
    const int64_t j = j0 + q * MS_THREADS + threadIdx.x;
    if (j < j1) {
      dst[j] = v[q];
      if (j >= new_carry && j - new_carry < L) carry_out[j - new_carry] = v[q];
    }
  }
}

template <typename T>
static int32_t launch_assemble(const T *d_chunks, T *d_pool, int64_t capacity, int32_t frame_length,
                               const int64_t *d_meta, const int64_t *d_tile_prefix, int32_t n, int64_t total_tiles,
                               T *d_work, void *stream) {
  if (n < 0 || total_tiles < 0 || capacity < 0 || frame_length <= 0) return invalid_ms("multistream_assemble: bad size");
  if (n == 0 || total_tiles == 0) return PDS_OK;
  if (total_tiles > 0x7fffffff) return invalid_ms("multistream_assemble: too many tiles in one call");
  if (!d_pool || !d_meta || !d_tile_prefix || !d_work) return invalid_ms("multistream_assemble: null pointer");
  hipLaunchKernelGGL(multistream_assemble_kernel<T>, dim3((unsigned)total_tiles), dim3(MS_THREADS), 0,
                     (hipStream_t)stream, d_chunks, d_pool, capacity, frame_length, d_meta, d_tile_prefix, n, d_work);
  PDS_HIP(hipGetLastError());
  return PDS_OK;
}

}  // namespace pds

extern "C" {

int32_t pds_multistream_tile(void) { return (int32_t)pds::MS_TILE; }

int32_t pds_multistream_assemble_f32(const float *d_chunks, float *d_pool, int64_t capacity, int32_t frame_length,
                                     const int64_t *d_meta, const int64_t *d_tile_prefix, int32_t n,
                                     int64_t total_tiles, float *d_work, void *stream) {
  return pds::launch_assemble<float>(d_chunks, d_pool, capacity, frame_length, d_meta, d_tile_prefix, n, total_tiles,
                                     d_work, stream);
}
int32_t pds_multistream_assemble_f64(const double *d_chunks, double *d_pool, int64_t capacity, int32_t frame_length,
                                     const int64_t *d_meta, const int64_t *d_tile_prefix, int32_t n,
                                     int64_t total_tiles, double *d_work, void *stream) {
  return pds::launch_assemble<double>(d_chunks, d_pool, capacity, frame_length, d_meta, d_tile_prefix, n, total_tiles,
                                      d_work, stream);
}

}  // extern "C"
