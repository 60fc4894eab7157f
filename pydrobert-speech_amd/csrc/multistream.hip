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
//
// PCM chunks and pre-emphasis across ticks (StreamBatch(preemphasis=...), int16 chunks): multistream_assemble_pcm_kernel,
// the same work with the chunk's sample type C apart from the working type T (int16 converted at the load, exact) and,
// with PRE, every chunk sample pre-emphasised on its way into the span: x - coeff * its predecessor in the stream's raw
// signal, pre.hip's arithmetic.  The predecessor of chunk sample ci >= 1 is chunk sample ci - 1 (dropped or not), that of
// ci = 0 the stream's previous raw sample, kept in a second ping-pong pool T[2][capacity] -- if the stream has had a
// sample since its start (bit MS_SEEN of the half word); without one the sample passes unchanged.  Carried samples are
// work values and pass untouched.  An entry without a work span (a chunk dropped whole, an empty one) has no tile but
// still hands its previous sample on: behind the tiles the grid has one lane per entry that writes the entry's new
// previous sample (the chunk's last raw sample, or the old one under an empty chunk) to the other half.  Tiles and lanes
// read the half the metadata names and write the other, so no block reads what another block of the launch writes.
//
// Dither across ticks (StreamBatch(dither=...)): multistream_assemble_dither_kernel, the PCM kernel with every chunk
// sample dithered first -- pre.hip::dither_kernel's noise (dither_noise.h) for the sample's position in the stream's raw
// signal under the utterance's key, both from a second metadata section int64[n][2] (position of the chunk's first
// sample, key) -- and, with a pre-emphasis, pre-emphasised against its dithered predecessor (the reference's order:
// dither, then pre-emphasis).  A tile works in two phases.  Phase 1: its lanes take the whole sample pairs that cover the
// tile's chunk samples and the one predecessor a pre-emphasis needs, one Philox block, logarithm, square root and
// sincospi per pair, and write the dithered values to LDS (at most MS_TILE + 2 of them).  Phase 2, after one barrier:
// the PCM kernel's loop with chunk values and predecessors read from LDS.  The previous-sample pool holds dithered
// samples: the lanes behind the tiles compute the noise of the chunk's last sample themselves.  Carried samples pass
// untouched.
//
// Delta features across ticks (StreamBatch(deltas=...)): multistream_deltas_kernel, after the STFT launches of a tick.
// Every stream of the tick is one entry of `meta` (int64[n][MD_FIELDS]).  Its virtual sequence is its `valid` history
// rows (pool half h) followed by its `fresh` new static rows; the entry's output rows are rows first .. first + rows of
// that sequence with their deltas, every tap's row index clamped to the sequence ("edge" padding at a stream's start
// and, for an entry with the final flag, at its end), and its next history is the sequence's last keep = min(valid +
// fresh, hist_rows) rows, written to the other half (final: keep = 0, the stream is reset).  Work is dealt by element:
// an entry has (rows + keep) * coeffs of them, `elem_prefix` their exclusive prefix sum, and lane g of the grid takes element g -- adjacent lanes hold adjacent coefficients of one row, whether a tick
// brings thousands of streams one frame each or one stream thousands of frames.
//
// Running / global CMVN across ticks (StreamBatch(cmvn=...)): multistream_cmvn_kernel, after the feature launches of a
// tick and before its deltas, in place on the tick's statics.  Every stream of the tick is one entry of `meta`
// (int64[n][MC_FIELDS]); one thread per (entry, coefficient), adjacent lanes adjacent coefficients, walks the entry's
// new rows in order: running, it adds the row to the coefficient's sums (float64: sum, sum of squares, kept per stream
// in a pool double[capacity][2][coeffs]; a fresh stream starts from the prior table instead of reading the pool), then
// normalises the row by the sums so far -- Standardize.accumulate(frame); Standardize.apply(frame) of the reference,
// operation for operation; global, it normalises every row by the prior's mean and scale, computed once.  A
// (stream, coefficient) pair belongs to one thread of the launch, which reads the pool once and writes it once, so the
// pool needs no second half.
//
// Frame stacking across ticks (StreamBatch(stack=...)): multistream_stack_kernel, the last launch of a tick.  Every
// stream of the tick is one entry of `meta` (int64[n][MK_FIELDS]).  Its virtual sequence is its `pending` rows (pool
// half h: the rows of earlier ticks that did not fill a group, fewer than num_vectors) followed by its `fresh` new rows;
// the entry's output is the sequence's first groups * num_vectors rows, which laid side by side in groups of
// num_vectors are the same values in the same order -- row q of the sequence is elements q * C .. of the entry's output
// --, and its next pending rows are the rest, written to the other half (final: none, the stream is reset).  A final
// entry under a padding has one group more than the sequence fills: rows past its end are the fill value or the
// sequence's last row.  Work is dealt by element as for the deltas.  Values are loaded and stored, never computed with,
// so NaN payloads and signed zeros pass.
#include "pds_internal.h"
#include "dither_noise.h"

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

enum { MS_SEEN = 2 };  // of the MS_HALF word (bit 0: the pool half): the stream has had a sample since its start

template <typename C, typename T, bool PRE>
__global__ __launch_bounds__(MS_THREADS) void multistream_assemble_pcm_kernel(
    const C *__restrict__ chunks, T *__restrict__ pool, int64_t capacity, int32_t L,
    const int64_t *__restrict__ meta, const int64_t *__restrict__ tile_prefix, int32_t n, int64_t total_tiles,
    T *__restrict__ work, double coeff, T *__restrict__ prev) {
  const int64_t tile = blockIdx.x;
  if (PRE && tile >= total_tiles) {  // behind the tiles: one lane per entry, the entry's new previous sample
    const int64_t e = (tile - total_tiles) * MS_THREADS + threadIdx.x;
    if (e >= n) return;
    const int64_t *m = meta + e * MS_FIELDS;
    const int64_t s = m[MS_STREAM], len = m[MS_CHUNK_LEN], half = m[MS_HALF] & 1;
    prev[(1 - half) * capacity + s] = len > 0 ? (T)chunks[m[MS_CHUNK_OFF] + len - 1] : prev[half * capacity + s];
    return;
  }
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
  const int64_t first = m[MS_DROP] > 0 ? -1 : carry_len;  // the work sample whose predecessor is not in the chunk
  const int64_t half = m[MS_HALF] & 1;
  const bool seen = (m[MS_HALF] & MS_SEEN) != 0;
  const T *carry_in = pool + (half * capacity + s) * (int64_t)L;
  T *carry_out = pool + ((1 - half) * capacity + s) * (int64_t)L;
  T *dst = work + m[MS_WORK_OFF];
  const int64_t j0 = (tile - tile_prefix[lo]) * MS_TILE;
  const int64_t j1 = j0 + MS_TILE < avail ? j0 + MS_TILE : avail;
  // loads of the tile first, then the stores (four independent loads in flight per lane, and with PRE their four
  // predecessors: the cache lines of the neighbouring lane's own load).  Chunk samples stay in their own type until
  // every load is issued: a conversion beside the load would wait for it
  const T before = PRE ? prev[half * capacity + s] : T(0);  // the stream's previous raw sample (if it has one)
  T v[MS_PER_THREAD];
  typename std::conditional<sizeof(C) < 4, int32_t, C>::type x[MS_PER_THREAD], p[MS_PER_THREAD];  // (whole registers)
#pragma unroll
  for (int q = 0; q < MS_PER_THREAD; ++q) {
    const int64_t j = j0 + q * MS_THREADS + threadIdx.x;
    v[q] = j < j1 && j < carry_len ? carry_in[j] : T(0);
    x[q] = j < j1 && j >= carry_len ? chunks[chunk_at + j] : C(0);
    if (PRE) p[q] = j < j1 && j >= carry_len && j != first ? chunks[chunk_at + j - 1] : C(0);
  }
#pragma unroll
  for (int q = 0; q < MS_PER_THREAD; ++q) {  // (the conversions stay behind the loads)
    asm volatile("" : "+v"(x[q]));
    if (PRE) asm volatile("" : "+v"(p[q]));
  }
#pragma unroll
  for (int q = 0; q < MS_PER_THREAD; ++q) {
    const int64_t j = j0 + q * MS_THREADS + threadIdx.x;
    if (j < j1) {
      if (j >= carry_len) {
        v[q] = (T)x[q];
        // pre.hip::preemph_kernel's arithmetic (float64, multiply and subtract rounded separately); a stream's first
        // sample has no predecessor and passes unchanged
        if (PRE && (j != first || seen))
          v[q] = (T)__dsub_rn((double)v[q], __dmul_rn(coeff, (double)(j != first ? (T)p[q] : before)));
      }
      dst[j] = v[q];
      if (j >= new_carry && j - new_carry < L) carry_out[j - new_carry] = v[q];
    }
  }
}

template <typename C, typename T>
static int32_t launch_assemble_pcm(const void *d_chunks, void *d_pool, int64_t capacity, int32_t frame_length,
                                   const int64_t *d_meta, const int64_t *d_tile_prefix, int32_t n, int64_t total_tiles,
                                   void *d_work, double preemph, void *d_prev, void *stream) {
  const bool pre = preemph != 0.0;
  // (with a pre-emphasis every entry takes part, whether it has a tile or not)
  const int64_t blocks = total_tiles + (pre ? ((int64_t)n + MS_THREADS - 1) / MS_THREADS : 0);
  if (n == 0 || blocks == 0) return PDS_OK;
  if (blocks > 0x7fffffff) return invalid_ms("multistream_assemble_pcm: too many tiles in one call");
  if (!d_pool || !d_meta || !d_tile_prefix || !d_work || (pre && !d_prev))
    return invalid_ms("multistream_assemble_pcm: null pointer");
  if (pre)
    hipLaunchKernelGGL((multistream_assemble_pcm_kernel<C, T, true>), dim3((unsigned)blocks), dim3(MS_THREADS), 0,
                       (hipStream_t)stream, (const C *)d_chunks, (T *)d_pool, capacity, frame_length, d_meta,
                       d_tile_prefix, n, total_tiles, (T *)d_work, preemph, (T *)d_prev);
  else
    hipLaunchKernelGGL((multistream_assemble_pcm_kernel<C, T, false>), dim3((unsigned)blocks), dim3(MS_THREADS), 0,
                       (hipStream_t)stream, (const C *)d_chunks, (T *)d_pool, capacity, frame_length, d_meta,
                       d_tile_prefix, n, total_tiles, (T *)d_work, preemph, (T *)d_prev);
  PDS_HIP(hipGetLastError());
  return PDS_OK;
}

// One kernel per working type: the chunk's type (T itself or int16) and the pre-emphasis are launch-wide flags, not
// template parameters, and the noise is computed at one place in the code -- beside a Philox block, a logarithm, a
// square root and a sincospi in float64 the branches cost nothing, and each further copy of that arithmetic is some
// 2.5 KB of device code (tests/test_resources.py bounds the library's).
template <typename T>
__global__ __launch_bounds__(MS_THREADS) void multistream_assemble_dither_kernel(
    const void *__restrict__ chunks, int32_t i16, T *__restrict__ pool, int64_t capacity, int32_t L,
    const int64_t *__restrict__ meta, const int64_t *__restrict__ tile_prefix, int32_t n, int64_t total_tiles,
    T *__restrict__ work, double coeff, T *__restrict__ prev, const int64_t *__restrict__ dmeta, double dither) {
  __shared__ T noisy[MS_TILE + 2];  // dithered chunk samples of the tile, by position in the raw signal from `base`
  const bool pre = coeff != 0.0;
  const int64_t tile = blockIdx.x;
  // behind the tiles (with a pre-emphasis only): one lane per entry, the entry's new (dithered) previous sample
  const bool lanes = tile >= total_tiles;
  int64_t e;
  if (lanes) {
    e = (tile - total_tiles) * MS_THREADS + threadIdx.x;
    if (e >= n) return;
  } else {  // entry of this tile: the last e with tile_prefix[e] <= tile (entries without samples have no tile)
    int lo = 0, hi = n;
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (tile_prefix[mid] <= tile) lo = mid; else hi = mid;
    }
    e = lo;
  }
  const int64_t *m = meta + e * MS_FIELDS;
  const int64_t s = m[MS_STREAM], len = m[MS_CHUNK_LEN], carry_len = m[MS_CARRY_LEN], new_carry = m[MS_NEW_CARRY];
  const int64_t drop = m[MS_DROP], chunk_off = m[MS_CHUNK_OFF];
  const int64_t avail = carry_len + len - drop;
  const int64_t half = m[MS_HALF] & 1;
  const bool seen = (m[MS_HALF] & MS_SEEN) != 0;
  const int64_t pos = dmeta[2 * e];  // chunk sample ci is sample pos + ci of the stream's raw signal
  const uint64_t key = (uint64_t)dmeta[2 * e + 1];
  const int64_t ci_at = drop - carry_len;  // work sample j >= carry_len is chunk sample ci_at + j
  const int64_t j0 = lanes ? 0 : (tile - tile_prefix[e]) * MS_TILE;
  const int64_t j1 = j0 + MS_TILE < avail ? j0 + MS_TILE : avail;
  // phase 1.  A tile dithers chunk samples [ca, cb): its own (at most MS_TILE) and, with a pre-emphasis, the one before
  // them; the pairs that cover their positions start at the even position `base` and number at most MS_TILE / 2 + 2,
  // dealt to the lanes in turn.  A lane behind the tiles dithers the chunk's last sample: one pair of its own
  int64_t ca, cb;
  if (lanes) {
    ca = len - 1, cb = len;
  } else {
    const int64_t cfirst = ci_at + (j0 > carry_len ? j0 : carry_len);
    ca = pre && cfirst > 0 ? cfirst - 1 : cfirst, cb = ci_at + j1;
  }
  const int64_t base = (pos + (ca > 0 ? ca : 0)) & ~(int64_t)1;
  const int64_t npairs = cb > ca && cb > 0 ? ((pos + cb - 1) >> 1) - (base >> 1) + 1 : 0;
  const int64_t mine = lanes ? 0 : threadIdx.x;  // this lane's first pair
  for (int64_t p = mine; p < npairs; p += MS_THREADS) {
    const int64_t c0 = base + 2 * p - pos, c1 = c0 + 1;  // the pair's chunk samples (either may lie outside [ca, cb))
    const bool in0 = c0 >= ca && c0 < cb, in1 = c1 >= ca && c1 < cb;
    T x0 = T(0), x1 = T(0);  // (the loads before the arithmetic; int16 is widened exactly)
    if (i16) {
      const int16_t *x = (const int16_t *)chunks + chunk_off;
      if (in0) x0 = (T)x[c0];
      if (in1) x1 = (T)x[c1];
    } else {
      const T *x = (const T *)chunks + chunk_off;
      if (in0) x0 = x[c0];
      if (in1) x1 = x[c1];
    }
    double even, odd;
    dither_pair((base >> 1) + p, key, dither, even, odd);
    const T y0 = dither_add<T>((double)x0, even), y1 = dither_add<T>((double)x1, odd);
    if (lanes) {
      prev[(1 - half) * capacity + s] = in0 ? y0 : y1;
    } else {
      if (in0) noisy[2 * p] = y0;
      if (in1) noisy[2 * p + 1] = y1;
    }
  }
  if (lanes) {  // (an empty chunk hands the old value on)
    if (len <= 0) prev[(1 - half) * capacity + s] = prev[half * capacity + s];
    return;
  }
  const T *carry_in = pool + (half * capacity + s) * (int64_t)L;
  T *carry_out = pool + ((1 - half) * capacity + s) * (int64_t)L;
  T *dst = work + m[MS_WORK_OFF];
  const T before = pre ? prev[half * capacity + s] : T(0);  // the stream's previous (dithered) sample, if it has one
  __syncthreads();
  // phase 2: the PCM kernel's loop over the dithered values (not unrolled: beside phase 1 the loads' latency is nothing)
  const int64_t at = pos - base;  // noisy[at + ci] is chunk sample ci
#pragma unroll 1
  for (int64_t j = j0 + threadIdx.x; j < j1; j += MS_THREADS) {
    T v;
    if (j < carry_len) {
      v = carry_in[j];
    } else {
      const int64_t ci = ci_at + j;
      v = noisy[at + ci];
      // pre.hip::preemph_kernel's arithmetic over the dithered signal; a stream's first sample passes unchanged
      if (pre && (ci > 0 || seen))
        v = (T)__dsub_rn((double)v, __dmul_rn(coeff, (double)(ci > 0 ? noisy[at + ci - 1] : before)));
    }
    dst[j] = v;
    if (j >= new_carry && j - new_carry < L) carry_out[j - new_carry] = v;
  }
}

template <typename T>
static int32_t launch_assemble_dither(const void *d_chunks, bool i16, void *d_pool, int64_t capacity,
                                      int32_t frame_length, const int64_t *d_meta, const int64_t *d_tile_prefix,
                                      int32_t n, int64_t total_tiles, void *d_work, double preemph, void *d_prev,
                                      const int64_t *d_dither, double dither, void *stream) {
  const bool pre = preemph != 0.0;
  // (with a pre-emphasis every entry takes part, whether it has a tile or not)
  const int64_t blocks = total_tiles + (pre ? ((int64_t)n + MS_THREADS - 1) / MS_THREADS : 0);
  if (n == 0 || blocks == 0) return PDS_OK;
  if (blocks > 0x7fffffff) return invalid_ms("multistream_assemble_dither: too many tiles in one call");
  if (!d_pool || !d_meta || !d_tile_prefix || !d_work || !d_dither || (pre && !d_prev))
    return invalid_ms("multistream_assemble_dither: null pointer");
  hipLaunchKernelGGL(multistream_assemble_dither_kernel<T>, dim3((unsigned)blocks), dim3(MS_THREADS), 0,
                     (hipStream_t)stream, d_chunks, (int32_t)i16, (T *)d_pool, capacity, frame_length, d_meta,
                     d_tile_prefix, n, total_tiles, (T *)d_work, preemph, (T *)d_prev, d_dither, dither);
  PDS_HIP(hipGetLastError());
  return PDS_OK;
}

// ---- delta features across ticks ------------------------------------------------------------------------------

enum { MD_STREAM = 0, MD_FLAGS, MD_VALID, MD_FRESH, MD_STATIC_ROW, MD_FIRST, MD_ROWS, MD_OUT_ROW, MD_FIELDS };
enum { MD_FLAG_HALF = 1, MD_FLAG_FINAL = 2 };
constexpr int MD_THREADS = 256;

template <typename T>
__global__ __launch_bounds__(MD_THREADS) void multistream_deltas_kernel(
    const T *__restrict__ statics, T *hist, int64_t capacity, int32_t hist_rows, int32_t F,
    const double *__restrict__ filts, const int32_t *__restrict__ filt_off, int32_t K,
    const int64_t *__restrict__ meta, const int64_t *__restrict__ elem_prefix, int32_t n, int64_t total,
    T *__restrict__ out) {
  const int64_t g = (int64_t)blockIdx.x * MD_THREADS + threadIdx.x;
  if (g >= total) return;
  // entry of this element: the last e with elem_prefix[e] <= g (entries without elements are passed over)
  int lo = 0, hi = n;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (elem_prefix[mid] <= g) lo = mid; else hi = mid;
  }
  const int64_t *m = meta + (int64_t)lo * MD_FIELDS;
  const int64_t s = m[MD_STREAM], half = m[MD_FLAGS] & MD_FLAG_HALF, valid = m[MD_VALID], rows = m[MD_ROWS];
  const int64_t V = valid + m[MD_FRESH];  // (> 0: an entry with elements has a row to show or to keep)
  const int64_t slot = (int64_t)hist_rows * F;
  const T *hin = hist + (half * capacity + s) * slot;
  const int64_t fresh_at = m[MD_STATIC_ROW] - valid;  // statics row of row v >= valid of the sequence: fresh_at + v
  const int64_t l = g - elem_prefix[lo];
  const int64_t r = l / F;
  const int i = (int)(l - r * F);
  auto row = [&](int64_t v) -> T {
    v = v < 0 ? 0 : (v >= V ? V - 1 : v);
    return v < valid ? hin[v * F + i] : statics[(fresh_at + v) * F + i];
  };
  if (r >= rows) {  // a row of the next history: the sequence's last min(V, hist_rows) rows (none after a finalize)
    if (m[MD_FLAGS] & MD_FLAG_FINAL) return;
    const int64_t q = r - rows, keep = V < hist_rows ? V : hist_rows;
    hist[((1 - half) * capacity + s) * slot + q * F + i] = row(V - keep + q);
    return;
  }
  const int64_t p = m[MD_FIRST] + r;
  T *orow = out + (m[MD_OUT_ROW] + r) * ((int64_t)(K + 1) * F) + i;
  orow[0] = row(p);
  for (int k = 1; k <= K; ++k) {
    const int f0 = filt_off[k - 1], len = filt_off[k] - f0;
    const int M = (len - 1) / 2;
    double acc = 0.0;
    // post.hip's arithmetic: multiply and add rounded separately (the Makefile builds this file without contraction)
    for (int j = 0; j < len; ++j) acc = __dadd_rn(acc, __dmul_rn(filts[f0 + j], (double)row(p + j - M)));
    orow[(int64_t)k * F] = (T)acc;
  }
}

template <typename T>
static int32_t launch_ms_deltas(const T *d_statics, T *d_hist, int64_t capacity, int32_t hist_rows, int32_t coeffs,
                                const double *d_filts, const int32_t *d_filt_off, int32_t K, const int64_t *d_meta,
                                const int64_t *d_elem_prefix, int32_t n, int64_t total_elems, T *d_out, void *stream) {
  if (n < 0 || total_elems < 0 || capacity < 0 || hist_rows <= 0 || coeffs <= 0 || K < 1)
    return invalid_ms("multistream_deltas: bad size");
  if (n == 0 || total_elems == 0) return PDS_OK;
  const int64_t blocks = (total_elems + MD_THREADS - 1) / MD_THREADS;
  if (blocks > 0x7fffffff) return invalid_ms("multistream_deltas: too many elements in one call");
  // (d_statics / d_out may be null in a tick without new rows / without rows due: only histories move)
  if (!d_hist || !d_filts || !d_filt_off || !d_meta || !d_elem_prefix)
    return invalid_ms("multistream_deltas: null pointer");
  hipLaunchKernelGGL(multistream_deltas_kernel<T>, dim3((unsigned)blocks), dim3(MD_THREADS), 0, (hipStream_t)stream,
                     d_statics, d_hist, capacity, hist_rows, coeffs, d_filts, d_filt_off, K, d_meta, d_elem_prefix, n,
                     total_elems, d_out);
  PDS_HIP(hipGetLastError());
  return PDS_OK;
}

// ---- running / global CMVN across ticks -----------------------------------------------------------------------

enum { MC_STREAM = 0, MC_FLAGS, MC_ROW, MC_ROWS, MC_COUNT, MC_FIELDS = 8 };
enum { MC_FLAG_FRESH = 1 };
constexpr int MC_THREADS = 256;
constexpr int MC_AHEAD = 4;  // row loads in flight per thread (the sums are sequential, the loads are not)

// mean and scale of one coefficient from its sums and count: Standardize._apply_vector's arithmetic (float64, every
// operation rounded separately; fabs(var) <= 1e-8 is numpy.isclose(var, 0), false for NaN as there)
__device__ __forceinline__ void cmvn_mean_scale(double s1, double s2, double count, bool norm_var, double &mean,
                                                double &scale) {
  mean = s1 / count;
  scale = 1.0;
  if (norm_var) {
    double var = __dsub_rn(s2 / count, __dmul_rn(mean, mean));
    if (fabs(var) <= 1e-8) var = 1.0;
    scale = 1.0 / sqrt(var);
  }
}

template <typename T>
__global__ __launch_bounds__(MC_THREADS) void multistream_cmvn_kernel(
    T *__restrict__ statics, double *__restrict__ pool, int64_t capacity, int32_t F,
    const double *__restrict__ prior, int32_t norm_var, int32_t running, const int64_t *__restrict__ meta,
    int64_t total) {
  const int64_t g = (int64_t)blockIdx.x * MC_THREADS + threadIdx.x;
  if (g >= total) return;
  const int64_t e = g / F;
  const int i = (int)(g - e * F);
  const int64_t *m = meta + e * MC_FIELDS;
  const int64_t k = m[MC_ROWS];
  if (k <= 0) return;  // (nothing to normalise and, the sums being unchanged, nothing to write)
  double *sums = pool + (m[MC_STREAM] * 2) * (int64_t)F + i;  // (not touched unless running)
  double s1, s2;
  if (running && !(m[MC_FLAGS] & MC_FLAG_FRESH)) {
    s1 = sums[0];
    s2 = sums[F];
  } else {
    s1 = prior ? prior[i] : 0.0;
    s2 = prior ? prior[F + i] : 0.0;
  }
  T *x = statics + m[MC_ROW] * (int64_t)F + i;
  double mean, scale, shift = 0.0;
  if (!running) {  // fixed statistics: once per thread
    cmvn_mean_scale(s1, s2, (double)m[MC_COUNT], norm_var != 0, mean, scale);
    shift = __dmul_rn(mean, scale);
  }
  int64_t count = m[MC_COUNT];
  for (int64_t t = 0; t < k; t += MC_AHEAD) {
    T v[MC_AHEAD];
#pragma unroll
    for (int u = 0; u < MC_AHEAD; ++u) v[u] = t + u < k ? x[(t + u) * (int64_t)F] : T(0);
#pragma unroll
    for (int u = 0; u < MC_AHEAD; ++u) {
      if (t + u >= k) continue;
      const double d = (double)v[u];
      if (running) {  // accumulate(frame), then apply(frame)
        s1 = __dadd_rn(s1, d);
        s2 = __dadd_rn(s2, __dmul_rn(d, d));
        ++count;
        cmvn_mean_scale(s1, s2, (double)count, norm_var != 0, mean, scale);
        shift = __dmul_rn(mean, scale);
      }
      x[(t + u) * (int64_t)F] = (T)__dsub_rn(__dmul_rn(d, scale), shift);
    }
  }
  if (running) {
    sums[0] = s1;
    sums[F] = s2;
  }
}

template <typename T>
static int32_t launch_ms_cmvn(T *d_statics, double *d_pool, int64_t capacity, int32_t coeffs, const double *d_prior,
                              int32_t norm_var, int32_t running, const int64_t *d_meta, int32_t n, void *stream) {
  if (n < 0 || capacity < 0 || coeffs <= 0) return invalid_ms("multistream_cmvn: bad size");
  if (n == 0) return PDS_OK;
  const int64_t total = (int64_t)n * coeffs;
  const int64_t blocks = (total + MC_THREADS - 1) / MC_THREADS;
  if (blocks > 0x7fffffff) return invalid_ms("multistream_cmvn: too many elements in one call");
  // (d_statics may be null in a tick without new rows: no entry has any then)
  if (!d_meta || (running && !d_pool)) return invalid_ms("multistream_cmvn: null pointer");
  hipLaunchKernelGGL(multistream_cmvn_kernel<T>, dim3((unsigned)blocks), dim3(MC_THREADS), 0, (hipStream_t)stream,
                     d_statics, d_pool, capacity, coeffs, d_prior, norm_var, running, d_meta, total);
  PDS_HIP(hipGetLastError());
  return PDS_OK;
}

// ---- frame stacking across ticks ------------------------------------------------------------------------------

enum { MK_STREAM = 0, MK_FLAGS, MK_PENDING, MK_FRESH, MK_ROW, MK_GROUPS, MK_OUT_ROW, MK_FIELDS = 8 };
enum { MK_FLAG_HALF = 1, MK_FLAG_FINAL = 2 };
enum { MK_PAD_NONE = 0, MK_PAD_CONSTANT = 1, MK_PAD_EDGE = 2 };
constexpr int MK_THREADS = 256;

template <typename T>
__global__ __launch_bounds__(MK_THREADS) void multistream_stack_kernel(
    const T *__restrict__ rows, T *pool, int64_t capacity, int32_t nv, int32_t C, const int64_t *__restrict__ meta,
    const int64_t *__restrict__ elem_prefix, int32_t n, int64_t total, int32_t pad, T fill, T *__restrict__ out) {
  const int64_t g = (int64_t)blockIdx.x * MK_THREADS + threadIdx.x;
  if (g >= total) return;
  // entry of this element: the last e with elem_prefix[e] <= g (entries without elements are passed over)
  int lo = 0, hi = n;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (elem_prefix[mid] <= g) lo = mid; else hi = mid;
  }
  const int64_t *m = meta + (int64_t)lo * MK_FIELDS;
  const int64_t s = m[MK_STREAM], half = m[MK_FLAGS] & MK_FLAG_HALF, pending = m[MK_PENDING];
  const int64_t V = pending + m[MK_FRESH];  // (> 0: an entry with elements has a row to show or to keep)
  const int64_t slot = (int64_t)(nv - 1) * C;
  const T *pin = pool + (half * capacity + s) * slot;
  const int64_t fresh_at = m[MK_ROW] - pending;  // `rows` row of row v >= pending of the sequence: fresh_at + v
  const int64_t l = g - elem_prefix[lo];
  const int64_t q = l / C;  // row of the sequence, or past its end in a padded last group
  const int i = (int)(l - q * C);
  auto row = [&](int64_t v) -> T { return v < pending ? pin[v * C + i] : rows[(fresh_at + v) * C + i]; };
  const int64_t shown = m[MK_GROUPS] * nv;
  if (q >= shown) {  // a row of the next pending ones: the sequence's rows behind the groups (none after a finalize)
    if (m[MK_FLAGS] & MK_FLAG_FINAL) return;
    pool[((1 - half) * capacity + s) * slot + (q - shown) * C + i] = row(q);
    return;
  }
  // (rows of one group lie side by side: the entry's output is its sequence, element for element)
  out[m[MK_OUT_ROW] * ((int64_t)nv * C) + l] = q < V ? row(q) : (pad == MK_PAD_EDGE ? row(V - 1) : fill);
}

template <typename T>
static int32_t launch_ms_stack(const T *d_rows, T *d_pool, int64_t capacity, int32_t num_vectors, int32_t coeffs,
                               const int64_t *d_meta, const int64_t *d_elem_prefix, int32_t n, int64_t total_elems,
                               int32_t pad, double fill, T *d_out, void *stream) {
  if (n < 0 || total_elems < 0 || capacity < 0 || num_vectors < 2 || coeffs <= 0)
    return invalid_ms("multistream_stack: bad size");
  if (pad != MK_PAD_NONE && pad != MK_PAD_CONSTANT && pad != MK_PAD_EDGE)
    return invalid_ms("multistream_stack: pad must be 0 (none), 1 (constant) or 2 (edge)");
  if (n == 0 || total_elems == 0) return PDS_OK;
  const int64_t blocks = (total_elems + MK_THREADS - 1) / MK_THREADS;
  if (blocks > 0x7fffffff) return invalid_ms("multistream_stack: too many elements in one call");
  // (d_rows / d_out may be null in a tick without new rows / without a full group: only pending rows move)
  if (!d_pool || !d_meta || !d_elem_prefix) return invalid_ms("multistream_stack: null pointer");
  hipLaunchKernelGGL(multistream_stack_kernel<T>, dim3((unsigned)blocks), dim3(MK_THREADS), 0, (hipStream_t)stream,
                     d_rows, d_pool, capacity, num_vectors, coeffs, d_meta, d_elem_prefix, n, total_elems, pad, (T)fill,
                     d_out);
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

int32_t pds_multistream_assemble_pcm(int32_t chunk_format, int32_t work_format, const void *d_chunks, void *d_pool,
                                     int64_t capacity, int32_t frame_length, const int64_t *d_meta,
                                     const int64_t *d_tile_prefix, int32_t n, int64_t total_tiles, void *d_work,
                                     double preemph, void *d_prev, void *stream) {
  if (work_format != PDS_SAMPLES_F32 && work_format != PDS_SAMPLES_F64)
    return pds::invalid_ms("multistream_assemble_pcm: work_format must be PDS_SAMPLES_F32 or PDS_SAMPLES_F64");
  if (chunk_format != work_format && chunk_format != PDS_SAMPLES_I16)
    return pds::invalid_ms("multistream_assemble_pcm: chunk_format must be work_format or PDS_SAMPLES_I16");
  if (n < 0 || total_tiles < 0 || capacity < 0 || frame_length <= 0)
    return pds::invalid_ms("multistream_assemble_pcm: bad size");
  if (!(preemph == preemph) || preemph - preemph != 0.0)
    return pds::invalid_ms("multistream_assemble_pcm: preemph must be finite");
  const bool f64 = work_format == PDS_SAMPLES_F64;
  auto fn = chunk_format == PDS_SAMPLES_I16
                ? (f64 ? pds::launch_assemble_pcm<int16_t, double> : pds::launch_assemble_pcm<int16_t, float>)
                : (f64 ? pds::launch_assemble_pcm<double, double> : pds::launch_assemble_pcm<float, float>);
  return fn(d_chunks, d_pool, capacity, frame_length, d_meta, d_tile_prefix, n, total_tiles, d_work, preemph, d_prev,
            stream);
}

int32_t pds_multistream_assemble_dither(int32_t chunk_format, int32_t work_format, const void *d_chunks, void *d_pool,
                                        int64_t capacity, int32_t frame_length, const int64_t *d_meta,
                                        const int64_t *d_tile_prefix, int32_t n, int64_t total_tiles, void *d_work,
                                        double preemph, void *d_prev, const int64_t *d_dither, double dither,
                                        void *stream) {
  if (!(dither == dither) || dither - dither != 0.0)
    return pds::invalid_ms("multistream_assemble_dither: dither must be finite");
  if (dither == 0.0)
    return pds_multistream_assemble_pcm(chunk_format, work_format, d_chunks, d_pool, capacity, frame_length, d_meta,
                                        d_tile_prefix, n, total_tiles, d_work, preemph, d_prev, stream);
  if (work_format != PDS_SAMPLES_F32 && work_format != PDS_SAMPLES_F64)
    return pds::invalid_ms("multistream_assemble_dither: work_format must be PDS_SAMPLES_F32 or PDS_SAMPLES_F64");
  if (chunk_format != work_format && chunk_format != PDS_SAMPLES_I16)
    return pds::invalid_ms("multistream_assemble_dither: chunk_format must be work_format or PDS_SAMPLES_I16");
  if (n < 0 || total_tiles < 0 || capacity < 0 || frame_length <= 0)
    return pds::invalid_ms("multistream_assemble_dither: bad size");
  if (!(preemph == preemph) || preemph - preemph != 0.0)
    return pds::invalid_ms("multistream_assemble_dither: preemph must be finite");
  auto fn = work_format == PDS_SAMPLES_F64 ? pds::launch_assemble_dither<double> : pds::launch_assemble_dither<float>;
  return fn(d_chunks, chunk_format == PDS_SAMPLES_I16, d_pool, capacity, frame_length, d_meta, d_tile_prefix, n,
            total_tiles, d_work, preemph, d_prev, d_dither, dither, stream);
}

int32_t pds_multistream_deltas_f32(const float *d_statics, float *d_hist, int64_t capacity, int32_t hist_rows,
                                   int32_t coeffs, const double *d_filts, const int32_t *d_filt_off, int32_t K,
                                   const int64_t *d_meta, const int64_t *d_elem_prefix, int32_t n, int64_t total_elems,
                                   float *d_out, void *stream) {
  return pds::launch_ms_deltas<float>(d_statics, d_hist, capacity, hist_rows, coeffs, d_filts, d_filt_off, K, d_meta,
                                      d_elem_prefix, n, total_elems, d_out, stream);
}
int32_t pds_multistream_deltas_f64(const double *d_statics, double *d_hist, int64_t capacity, int32_t hist_rows,
                                   int32_t coeffs, const double *d_filts, const int32_t *d_filt_off, int32_t K,
                                   const int64_t *d_meta, const int64_t *d_elem_prefix, int32_t n, int64_t total_elems,
                                   double *d_out, void *stream) {
  return pds::launch_ms_deltas<double>(d_statics, d_hist, capacity, hist_rows, coeffs, d_filts, d_filt_off, K, d_meta,
                                       d_elem_prefix, n, total_elems, d_out, stream);
}

int32_t pds_multistream_cmvn_f32(float *d_statics, double *d_pool, int64_t capacity, int32_t coeffs,
                                 const double *d_prior, int32_t norm_var, int32_t running, const int64_t *d_meta,
                                 int32_t n, void *stream) {
  return pds::launch_ms_cmvn<float>(d_statics, d_pool, capacity, coeffs, d_prior, norm_var, running, d_meta, n, stream);
}
int32_t pds_multistream_cmvn_f64(double *d_statics, double *d_pool, int64_t capacity, int32_t coeffs,
                                 const double *d_prior, int32_t norm_var, int32_t running, const int64_t *d_meta,
                                 int32_t n, void *stream) {
  return pds::launch_ms_cmvn<double>(d_statics, d_pool, capacity, coeffs, d_prior, norm_var, running, d_meta, n, stream);
}

int32_t pds_multistream_stack_f32(const float *d_rows, float *d_pool, int64_t capacity, int32_t num_vectors,
                                  int32_t coeffs, const int64_t *d_meta, const int64_t *d_elem_prefix, int32_t n,
                                  int64_t total_elems, int32_t pad, double fill, float *d_out, void *stream) {
  return pds::launch_ms_stack<float>(d_rows, d_pool, capacity, num_vectors, coeffs, d_meta, d_elem_prefix, n,
                                     total_elems, pad, fill, d_out, stream);
}
int32_t pds_multistream_stack_f64(const double *d_rows, double *d_pool, int64_t capacity, int32_t num_vectors,
                                  int32_t coeffs, const int64_t *d_meta, const int64_t *d_elem_prefix, int32_t n,
                                  int64_t total_elems, int32_t pad, double fill, double *d_out, void *stream) {
  return pds::launch_ms_stack<double>(d_rows, d_pool, capacity, num_vectors, coeffs, d_meta, d_elem_prefix, n,
                                      total_elems, pad, fill, d_out, stream);
}

}  // extern "C"
