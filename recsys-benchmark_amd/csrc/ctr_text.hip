// ctr_text.hip — the Criteo text format on the device: a chunk of the file's bytes in, int64 keys, uint8 labels and
// int64 line numbers out, equal element for element to `read_criteo_text` of ctr_data.py on every file both accept
// (reference: src/dataset/criteo/criteo_torchfm.py, `__yield_buffer` / `convert_numeric_feature`).  The grammar is
// spelled out in include/mi355x_recsys.h.
//
// Index (mi_ctr_text_index), six launches, after the mark / scan-tiles / scatter pattern of ctr_data.hip:
//   count         a lane classifies 16 bytes (one aligned 16-byte load; the chunk's ragged ends byte by byte) and the tile
//                 of 4096 bytes writes its numbers of separators ('\t', '\n') and of newlines;
//   scan tiles    one workgroup turns both into exclusive offsets and writes the totals;
//   scatter       separator s of the chunk, in byte order, gets sep_pos[s] = its byte offset (bit 31: it is a newline),
//                 newline L gets nl_sep[L] = its separator number; the last newline gives the bytes consumed;
//   count lines   line L has nl_sep[L] - nl_sep[L-1] - 1 tabs; a tile of 256 lines counts those with exactly F of them;
//   scan lines    one workgroup: exclusive offsets, the record {lines, kept, consumed}, and the column of a '\r';
//   number lines  kept line k, in file order, gets kept_line[k] = L.
// The issue's sketch had three launches; a line's tab count is a difference of two neighbouring nl_sep entries, which the
// scatter itself writes, so deciding and numbering the kept lines takes a second count / scan / scatter round over lines.
// Every launch is a streaming pass or a single workgroup, and all six reuse block_excl_scan.
//
// Parse (mi_ctr_text_parse), one launch: one lane per (kept line, column) reads its field's two separator positions, loads
// at most 19 bytes with loads that do not wait for one another, and converts them.  No lane walks a line.  The logarithm
// of `convert_numeric_feature` is not evaluated: the key of v > 2 is the number of entries <= v of the caller's threshold
// table, one binary search.
//
// Other delimited formats (mi_ctr_table_index / mi_ctr_table_parse: Avazu's comma-separated file with a header, KDD 2012
// track 2's tab-separated one; src/dataset/avazu/avazu_on_ram.py, src/dataset/kdd/kdd_dataset.py) run the SAME six index
// kernels, which take the separator byte and the number of header lines (never kept, never counted) from their argument
// record, and one parse kernel that converts a field by the kind its column has in a caller's spec (k_table_parse).
//
// Integer arithmetic and plain vector stores only; no arrival order enters any value, so reruns give the same bits.
// The only atomics are on the error path: the OR into the error word (a subscript that fails its check: never with a
// workspace this file wrote), the 64-bit minimum that keeps the lowest offending (line, column) in *err_record, and the
// 64-bit minimum over (line, separators before it) of the '\r' bytes, from which scan lines derives that column.
// Every byte subscript is checked against nbytes, every workspace subscript against its capacity, before it is used.
#include "common.hpp"

namespace {
using namespace mi;

constexpr int kLaneBytes = 16;
constexpr int kTileBytes = kBlock * kLaneBytes;
constexpr uint32_t kNewlineBit = 0x80000000u, kPosMask = 0x7FFFFFFFu;
constexpr int kMaxDigits = 18, kMaxHex = 15, kColBits = 16;
constexpr int64_t kNullKey = INT64_MIN, kEmptyKey = -1;
constexpr unsigned long long kNoError = ~0ull;

inline int64_t tiles_of(int64_t n) { return (n + kBlock - 1) / kBlock; }
inline int64_t align16(int64_t b) { return (b + 15) & ~(int64_t)15; }
inline int grid_for_tiles(int64_t tiles) { return (int)(tiles < 1 ? 1 : (tiles > kMaxGrid ? kMaxGrid : tiles)); }

// the workspace: totals {separators, lines, lowest '\r' as (line << 32 | separators before it), kept lines, header lines},
// then the arrays
struct Text {
  const uint8_t *text;
  int64_t nbytes, first_line_no;
  int64_t cap, kept_cap;                 // entries of sep_pos / nl_sep, of kept_line
  int64_t byte_tiles;
  int misalign, final, F;              // F: the separators of a kept line
  int sep, n_header;                     // the field separator byte; leading lines of the chunk never kept nor counted
  unsigned long long *totals;
  uint32_t *tile_seps, *tile_nls, *line_tiles, *sep_pos, *nl_sep, *kept_line;
  int64_t *record;
  unsigned long long *err_record;
  int *err;
};

int64_t lay_out(Text &t, void *workspace, int64_t nbytes, int F) {
  const uintptr_t base = reinterpret_cast<uintptr_t>(workspace);    // (null when only the size is asked for)
  t.cap = nbytes + 1;                                   // every byte a separator, and the newline a final line lacks
  t.kept_cap = t.cap / (F + 1) + 1;                     // a kept line owns F + 1 separators
  const int64_t byte_tiles = (nbytes + 1 + (kLaneBytes - 1) + kTileBytes - 1) / kTileBytes, line_tiles = tiles_of(t.cap);
  int64_t at = 0;
  auto take = [&](int64_t bytes) { int64_t here = at; at += align16(bytes); return base + (uintptr_t)here; };
  t.totals = reinterpret_cast<unsigned long long *>(take(5 * 8));
  t.tile_seps = reinterpret_cast<uint32_t *>(take(byte_tiles * 4));
  t.tile_nls = reinterpret_cast<uint32_t *>(take(byte_tiles * 4));
  t.line_tiles = reinterpret_cast<uint32_t *>(take(line_tiles * 4));
  t.sep_pos = reinterpret_cast<uint32_t *>(take(t.cap * 4));
  t.nl_sep = reinterpret_cast<uint32_t *>(take(t.cap * 4));
  t.kept_line = reinterpret_cast<uint32_t *>(take(t.kept_cap * 4));
  return at;
}

// a final chunk that does not end in '\n' gets one at offset nbytes
__device__ __forceinline__ bool virtual_newline(const Text &a) {
  return a.final && a.nbytes > 0 && a.text[a.nbytes - 1] != '\n';
}

struct Masks {
  uint32_t sep, nl, cr;                  // bit j: byte b0 + j is a separator / a newline / a '\r'
};

// bytes [b0, b0 + 16) of the chunk; b0 = 16 g - misalign, so text + b0 is 16-byte aligned
__device__ __forceinline__ Masks classify(const Text &a, int64_t b0, bool virt) {
  uint32_t w[4] = {0u, 0u, 0u, 0u};
  if (b0 >= 0 && b0 + kLaneBytes <= a.nbytes) {
    const uint4 v = *reinterpret_cast<const uint4 *>(a.text + b0);
    w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
  } else {
#pragma unroll
    for (int j = 0; j < kLaneBytes; ++j) {
      const int64_t p = b0 + j;
      if (p >= 0 && p < a.nbytes) w[j >> 2] |= (uint32_t)a.text[p] << (8 * (j & 3));
    }
  }
  Masks m = {0u, 0u, 0u};
#pragma unroll
  for (int j = 0; j < kLaneBytes; ++j) {
    const uint32_t ch = (w[j >> 2] >> (8 * (j & 3))) & 255u;
    m.nl |= (uint32_t)(ch == '\n') << j;
    m.sep |= (uint32_t)(ch == '\n' || ch == (uint32_t)a.sep) << j;
    m.cr |= (uint32_t)(ch == '\r') << j;
  }
  if (virt && b0 <= a.nbytes && a.nbytes < b0 + kLaneBytes) {
    m.nl |= 1u << (int)(a.nbytes - b0);
    m.sep |= 1u << (int)(a.nbytes - b0);
  }
  return m;
}

// a tile holds at most 4096 separators: both counts ride in one scanned word (separators low, newlines high)
__device__ __forceinline__ uint32_t packed_counts(const Masks &m) { return (uint32_t)__popc(m.sep) | ((uint32_t)__popc(m.nl) << 16); }

__global__ __launch_bounds__(kBlock) void k_text_count(Text a) {
  __shared__ uint32_t sm[kWavesPerBlock];
  const bool virt = virtual_newline(a);
  for (int64_t t = blockIdx.x; t < a.byte_tiles; t += gridDim.x) {
    const int64_t b0 = (t * kBlock + threadIdx.x) * kLaneBytes - a.misalign;
    uint32_t total;
    block_excl_scan(packed_counts(classify(a, b0, virt)), sm, &total);
    if (threadIdx.x == 0) {
      a.tile_seps[t] = total & 0xFFFFu;
      a.tile_nls[t] = total >> 16;
    }
  }
}

// one workgroup: both tile arrays become their exclusive scans; totals and the record's `consumed` are set up
__global__ __launch_bounds__(kBlock) void k_text_scan_tiles(Text a) {
  __shared__ uint32_t sm[kWavesPerBlock];
  uint32_t carry_s = 0, carry_n = 0;
  for (int64_t base = 0; base < a.byte_tiles; base += kBlock) {
    const int64_t i = base + threadIdx.x;
    const bool in = i < a.byte_tiles;
    uint32_t total;
    uint32_t before = block_excl_scan(in ? a.tile_seps[i] : 0u, sm, &total);
    if (in) a.tile_seps[i] = carry_s + before;
    carry_s += total;
    before = block_excl_scan(in ? a.tile_nls[i] : 0u, sm, &total);
    if (in) a.tile_nls[i] = carry_n + before;
    carry_n += total;
  }
  if (threadIdx.x == 0) {
    a.totals[0] = carry_s;
    a.totals[1] = carry_n;
    a.totals[2] = kNoError;
    a.totals[3] = 0;
    a.record[2] = 0;
  }
}

__global__ __launch_bounds__(kBlock) void k_text_scatter(Text a) {
  __shared__ uint32_t sm[kWavesPerBlock];
  const bool virt = virtual_newline(a);
  const int64_t n_lines = (int64_t)a.totals[1];
  for (int64_t t = blockIdx.x; t < a.byte_tiles; t += gridDim.x) {
    const int64_t b0 = (t * kBlock + threadIdx.x) * kLaneBytes - a.misalign;
    const Masks m = classify(a, b0, virt);
    uint32_t total;
    const uint32_t before = block_excl_scan(packed_counts(m), sm, &total);
    const int64_t s0 = (int64_t)a.tile_seps[t] + (before & 0xFFFFu), l0 = (int64_t)a.tile_nls[t] + (before >> 16);
    int64_t s = s0, l = l0;
    for (uint32_t left = m.sep; left; left &= left - 1) {
      const int j = __ffs(left) - 1;
      const int64_t p = b0 + j;                                        // 0 <= p <= nbytes < 2^31
      const bool nl = (m.nl >> j) & 1u;
      if (s < a.cap && (!nl || l < a.cap)) {
        a.sep_pos[s] = (uint32_t)p | (nl ? kNewlineBit : 0u);
        if (nl) {
          a.nl_sep[l] = (uint32_t)s;
          if (l == n_lines - 1) a.record[2] = p + 1 < a.nbytes ? p + 1 : a.nbytes;
        }
      } else if (a.err) {
        atomicOr(a.err, MI_IDX_OUT_OF_RANGE);
      }
      l += nl;
      ++s;
    }
    if (m.cr) {                                                        // error path: the first '\r' of these bytes
      const uint32_t below = (1u << (__ffs(m.cr) - 1)) - 1u;
      const int64_t line = l0 + __popc(m.nl & below), seps = s0 + __popc(m.sep & below);
      if (line < n_lines)                                              // (past the last newline: the next chunk's bytes)
        atomicMin(&a.totals[2], ((unsigned long long)line << 32) | (unsigned long long)seps);
    }
  }
}

// line l of the chunk is past the header and has exactly F field separators; l < n_lines <= cap
__device__ __forceinline__ bool line_kept(const Text &a, int64_t l) {
  const int64_t first = l ? (int64_t)a.nl_sep[l - 1] + 1 : 0;
  return l >= a.n_header && (int64_t)a.nl_sep[l] - first == a.F;
}

// the file's number of line l of the chunk: the header is not counted (an offence in it is named as the line after it)
__device__ __forceinline__ int64_t line_number(const Text &a, int64_t header, int64_t l) {
  return a.first_line_no + (l > header ? l - header : 0);
}

__global__ __launch_bounds__(kBlock) void k_text_count_lines(Text a) {
  __shared__ uint32_t sm[kWavesPerBlock];
  const int64_t n_lines = (int64_t)a.totals[1] < a.cap ? (int64_t)a.totals[1] : a.cap;
  const int64_t tiles = (n_lines + kBlock - 1) / kBlock;
  for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
    const int64_t l = t * kBlock + threadIdx.x;
    uint32_t total;
    block_excl_scan(l < n_lines && line_kept(a, l), sm, &total);
    if (threadIdx.x == 0) a.line_tiles[t] = total;
  }
}

// one workgroup: line_tiles becomes its exclusive scan; the record; the (line, column) of the chunk's first '\r'
__global__ __launch_bounds__(kBlock) void k_text_scan_lines(Text a) {
  __shared__ uint32_t sm[kWavesPerBlock];
  const int64_t n_lines = (int64_t)a.totals[1] < a.cap ? (int64_t)a.totals[1] : a.cap;
  const int64_t tiles = (n_lines + kBlock - 1) / kBlock;
  uint32_t carry = 0;
  for (int64_t base = 0; base < tiles; base += kBlock) {
    const int64_t i = base + threadIdx.x;
    uint32_t total;
    const uint32_t before = block_excl_scan(i < tiles ? a.line_tiles[i] : 0u, sm, &total);
    if (i < tiles) a.line_tiles[i] = carry + before;
    carry += total;
  }
  if (threadIdx.x == 0) {
    a.totals[3] = carry;
    a.totals[4] = (unsigned long long)a.n_header;
    a.record[0] = n_lines - (n_lines < a.n_header ? n_lines : a.n_header);
    a.record[1] = (int64_t)carry;
    const unsigned long long cr = a.totals[2];
    if (cr != kNoError) {
      const int64_t line = (int64_t)(cr >> 32), seps = (int64_t)(cr & 0xFFFFFFFFull);
      if (line < n_lines) {
        int64_t col = seps - (line ? (int64_t)a.nl_sep[line - 1] + 1 : 0);
        col = col < 0 ? 0 : (col > (1 << kColBits) - 1 ? (1 << kColBits) - 1 : col);
        atomicMin(a.err_record, ((unsigned long long)line_number(a, a.n_header, line) << kColBits) | (unsigned long long)col);
      }
    }
  }
}

__global__ __launch_bounds__(kBlock) void k_text_number_lines(Text a) {
  __shared__ uint32_t sm[kWavesPerBlock];
  const int64_t n_lines = (int64_t)a.totals[1] < a.cap ? (int64_t)a.totals[1] : a.cap;
  const int64_t tiles = (n_lines + kBlock - 1) / kBlock;
  for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
    const int64_t l = t * kBlock + threadIdx.x;
    const uint32_t kept = l < n_lines && line_kept(a, l);
    uint32_t total;
    const int64_t k = (int64_t)a.line_tiles[t] + block_excl_scan(kept, sm, &total);
    if (kept) {
      if (k < a.kept_cap) a.kept_line[k] = (uint32_t)l;
      else if (a.err) atomicOr(a.err, MI_IDX_OUT_OF_RANGE);
    }
  }
}

struct Parse {
  Text t;
  int64_t n_kept;
  int n_int;
  const int64_t *thresholds;
  int n_thresholds;
  int64_t *keys;
  uint8_t *labels;
  int64_t *line_no;
};

// A field's bytes, at most kFieldBytes of them (a longer field is in no column's grammar).  The loads do not depend on one
// another, so a lane waits for memory once per field, not once per byte; every loop below is unrolled with constant
// subscripts, which keeps `ch` in registers.
constexpr int kFieldBytes = kMaxDigits + 1;
struct Field {
  uint32_t ch[kFieldBytes];
  int len;                               // <= kFieldBytes
};

// false: not in the grammar
__device__ __forceinline__ bool parse_integer(const Parse &a, const Field &f, int64_t *key) {
  if (f.len == 0) {
    *key = kNullKey;
    return true;
  }
  const int neg = f.ch[0] == '-';
  if (f.len - neg < 1 || f.len - neg > kMaxDigits) return false;
  int64_t v = 0;
  bool digits = true;
#pragma unroll
  for (int i = 0; i < kFieldBytes; ++i) {
    if (i >= neg && i < f.len) {
      const uint32_t d = f.ch[i] - '0';
      digits = digits && d <= 9u;
      v = v * 10 + (d & 15u);                                           // < 16 * 10^18 / 9 < 2^63 whatever the bytes are
    }
  }
  if (!digits) return false;
  if (neg) v = -v;
  if (v <= 2) {
    *key = v - 2;
    return true;
  }
  int lo = 0, hi = a.n_thresholds;                                      // the number of thresholds <= v
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (a.thresholds[mid] <= v) lo = mid + 1; else hi = mid;
  }
  *key = lo;
  return true;
}

__device__ __forceinline__ bool parse_hex(const Field &f, int64_t *key) {
  if (f.len == 0) {
    *key = kEmptyKey;
    return true;
  }
  if (f.len > kMaxHex) return false;
  int64_t v = 0;
  bool digits = true;
#pragma unroll
  for (int i = 0; i < kMaxHex; ++i) {
    if (i < f.len) {
      const uint32_t ch = f.ch[i], lower = ch | 0x20u;
      const bool dec = ch - '0' <= 9u, alpha = lower - 'a' <= 5u;
      digits = digits && (dec || alpha);
      v = (v << 4) | (dec ? ch - '0' : (lower - 'a' + 10u) & 15u);       // < 2^60
    }
  }
  if (!digits) return false;
  *key = v;
  return true;
}

__global__ __launch_bounds__(kBlock) void k_text_parse(Parse a) {
  const Text &t = a.t;
  const int64_t w = t.F + 1, total = a.n_kept * w;
  const bool narrow = total <= (int64_t)UINT32_MAX;
  const int64_t n_seps = (int64_t)t.totals[0] < t.cap ? (int64_t)t.totals[0] : t.cap;
  const int64_t n_lines = (int64_t)t.totals[1] < t.cap ? (int64_t)t.totals[1] : t.cap;
  const int64_t kept = (int64_t)t.totals[3] < t.kept_cap ? (int64_t)t.totals[3] : t.kept_cap;
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < total; e += stride) {
    int64_t k;
    int c;
    if (narrow) {
      const uint32_t q = (uint32_t)e / (uint32_t)w;
      k = q;
      c = (int)((uint32_t)e - q * (uint32_t)w);
    } else {
      k = e / w;
      c = (int)(e - k * w);
    }
    // field c of kept line k lies between separators si - 1 and si
    bool ok = k < kept;
    const int64_t line = ok ? (int64_t)t.kept_line[k] : 0;
    ok = ok && line < n_lines;
    const int64_t si = (ok && line ? (int64_t)t.nl_sep[line - 1] + 1 : 0) + c;
    ok = ok && si < n_seps;
    const int64_t end = ok ? (int64_t)(t.sep_pos[si] & kPosMask) : 0;
    const int64_t begin = ok && si ? (int64_t)(t.sep_pos[si - 1] & kPosMask) + 1 : 0;
    ok = ok && begin <= end && end <= t.nbytes;
    int64_t key = 0;
    bool good = false;
    if (ok) {
      const bool fits = end - begin <= kFieldBytes;                       // a longer field is refused unread
      Field f;
      f.len = fits ? (int)(end - begin) : 0;
#pragma unroll
      for (int i = 0; i < kFieldBytes; ++i) f.ch[i] = i < f.len ? (uint32_t)t.text[begin + i] : 0u;   // begin + len <= nbytes
      if (!fits) {
        good = false;
      } else if (c == 0) {
        good = f.len == 1 && (f.ch[0] == '0' || f.ch[0] == '1');
        key = good ? (int64_t)(f.ch[0] - '0') : 0;
      } else if (c <= a.n_int) {
        good = parse_integer(a, f, &key);
      } else {
        good = parse_hex(f, &key);
      }
      if (!good) {
        key = 0;
        atomicMin(t.err_record, ((unsigned long long)(t.first_line_no + line) << kColBits) | (unsigned long long)c);
      }
    } else if (t.err) {
      atomicOr(t.err, MI_IDX_OUT_OF_RANGE);
    }
    if (c == 0) {
      a.labels[k] = (uint8_t)key;
      a.line_no[k] = ok ? t.first_line_no + line : -1;
    } else {
      a.keys[k * t.F + (c - 1)] = key;
    }
  }
}

// ---- the column-spec reader (mi_ctr_table_parse): the grammar of a column is a kind, not a position ---------------------
constexpr int kTableBytes = 20, kTokenBytes = 8, kLabelDigits = 18, kMaxCols = 256;
constexpr unsigned long long kMaxTenth = 1844674407370955161ull;         // (2^64 - 1) / 10; 2^64 - 1 ends in 5

struct TableParse {
  Text t;
  int64_t n_kept;
  const int32_t *spec;
  int derive_time;
  int64_t *keys;
  uint8_t *labels;
  int64_t *line_no;
};

// Monday = 0.  Days since 1970-01-01 (a Thursday) by the days-from-civil count over 400-year eras; y >= 1
__device__ __forceinline__ int weekday_of(int y, int m, int d) {
  y -= m <= 2;
  const int era = y / 400, yoe = y - era * 400;
  const int doy = (153 * (m > 2 ? m - 3 : m + 9) + 2) / 5 + d - 1;
  const int doe = yoe * 365 + yoe / 4 - yoe / 100 + doy;
  const int days = era * 146097 + doe - 719468;
  return (days + 3 + 7 * 146097) % 7;
}

__global__ __launch_bounds__(kBlock) void k_table_parse(TableParse a) {
  __shared__ uint32_t sm[kWavesPerBlock];
  const Text &t = a.t;
  const int64_t w = t.F + 1, total = a.n_kept * w;                        // w file columns, w <= kMaxCols = kBlock
  // F = the spec's number of key columns (low half), its number of TIME columns (high half): every workgroup counts them
  uint32_t mine = 0, counts;
  if ((int64_t)threadIdx.x < w) {
    const int kind = a.spec[threadIdx.x] & 255;
    mine = (uint32_t)(kind == MI_CTR_COL_TOKEN8 || kind == MI_CTR_COL_DEC64 || kind == MI_CTR_COL_TIME) |
           ((uint32_t)(kind == MI_CTR_COL_TIME) << 16);
  }
  block_excl_scan(mine, sm, &counts);
  const int F = (int)(counts & 0xFFFFu);
  const bool timed = a.derive_time != 0 && (counts >> 16) != 0;
  const int64_t F_out = F + (timed ? 3 : 0);
  const bool narrow = total <= (int64_t)UINT32_MAX;
  const int64_t n_seps = (int64_t)t.totals[0] < t.cap ? (int64_t)t.totals[0] : t.cap;
  const int64_t n_lines = (int64_t)t.totals[1] < t.cap ? (int64_t)t.totals[1] : t.cap;
  const int64_t kept = (int64_t)t.totals[3] < t.kept_cap ? (int64_t)t.totals[3] : t.kept_cap;
  const int64_t header = t.totals[4] ? 1 : 0;                             // what the index call was given
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < total; e += stride) {
    int64_t k;
    int c;
    if (narrow) {
      const uint32_t q = (uint32_t)e / (uint32_t)w;
      k = q;
      c = (int)((uint32_t)e - q * (uint32_t)w);
    } else {
      k = e / w;
      c = (int)(e - k * w);
    }
    const int32_t entry = a.spec[c];                                      // c < w
    const int kind = entry & 255;
    const int64_t oc = entry >> 8;
    const bool reads = kind != MI_CTR_COL_SKIP;
    // field c of kept line k lies between separators si - 1 and si
    bool ok = k < kept;
    const int64_t line = ok ? (int64_t)t.kept_line[k] : 0;
    ok = ok && line < n_lines;
    const int64_t si = (ok && line ? (int64_t)t.nl_sep[line - 1] + 1 : 0) + c;
    ok = ok && si < n_seps;
    const int64_t end = ok && reads ? (int64_t)(t.sep_pos[si] & kPosMask) : 0;
    const int64_t begin = ok && reads && si ? (int64_t)(t.sep_pos[si - 1] & kPosMask) + 1 : 0;
    ok = ok && begin <= end && end <= t.nbytes;
    const bool fits = end - begin <= kTableBytes;                         // a longer field is refused unread
    const int len = ok && reads && fits ? (int)(end - begin) : 0;
    uint32_t ch[kTableBytes];
#pragma unroll
    for (int i = 0; i < kTableBytes; ++i) ch[i] = i < len ? (uint32_t)t.text[begin + i] : 0u;     // begin + len <= nbytes
    // every reading of the bytes, whatever the kind: the kind picks among them below
    bool digits = true, printable = true;
    unsigned long long v = 0, token = 0;
    bool over = false;
#pragma unroll
    for (int i = 0; i < kTableBytes; ++i) {
      if (i < len) {
        const uint32_t d = ch[i] - '0';
        digits = digits && d <= 9u;
        if (i == kTableBytes - 1) over = v > kMaxTenth || (v == kMaxTenth && (d & 15u) > 5u);
        v = v * 10ull + (d & 15u);                                        // 19 digits: < 16 * 10^19 / 9 < 2^64
        if (i < kTokenBytes) {
          printable = printable && ch[i] - 0x21u <= 0x5Du;
          token |= (unsigned long long)ch[i] << (56 - 8 * i);
        }
      }
    }
    bool good = true;
    int64_t key = 0;
    int label = 0, hour = 0, weekday = 0;
    if (kind == MI_CTR_COL_LABEL01) {
      good = len == 1 && (ch[0] == '0' || ch[0] == '1');
      label = ch[0] == '1';
    } else if (kind == MI_CTR_COL_LABEL_COUNT) {
      good = len >= 1 && len <= kLabelDigits && digits;
      label = v >= 1ull;
    } else if (kind == MI_CTR_COL_TOKEN8 || kind == MI_CTR_COL_TIME) {
      good = len <= kTokenBytes && printable;
      key = (int64_t)token;
      if (kind == MI_CTR_COL_TIME && timed) {
        const int yy = (int)((ch[0] - '0') * 10 + (ch[1] - '0')), mm = (int)((ch[2] - '0') * 10 + (ch[3] - '0'));
        const int dd = (int)((ch[4] - '0') * 10 + (ch[5] - '0'));
        hour = (int)((ch[6] - '0') * 10 + (ch[7] - '0'));
        const int year = yy <= 68 ? 2000 + yy : 1900 + yy;
        const bool leap = (year % 4 == 0 && year % 100 != 0) || year % 400 == 0;
        const int month_days = mm == 2 ? 28 + (int)leap : 30 + ((mm + (mm >> 3)) & 1);
        good = len == 8 && digits && mm >= 1 && mm <= 12 && dd >= 1 && dd <= month_days && hour <= 23;
        weekday = good ? weekday_of(year, mm, dd) : 0;
      }
    } else if (kind == MI_CTR_COL_DEC64) {
      good = len >= 1 && digits && !(len > 1 && ch[0] == '0') && !over;
      key = (int64_t)v;
    } else if (kind != MI_CTR_COL_SKIP) {
      good = false;                                                       // no such kind: the column is refused
    }
    good = good && (fits || !reads);
    if (ok && !good) atomicMin(t.err_record, ((unsigned long long)line_number(t, header, line) << kColBits) | (unsigned long long)c);
    if (!ok && t.err) atomicOr(t.err, MI_IDX_OUT_OF_RANGE);
    if (!ok || !good) key = 0, label = 0, hour = 0, weekday = 0;
    if (c == 0) a.line_no[k] = ok ? line_number(t, header, line) : -1;
    if (kind == MI_CTR_COL_LABEL01 || kind == MI_CTR_COL_LABEL_COUNT) a.labels[k] = (uint8_t)label;
    if (kind == MI_CTR_COL_TOKEN8 || kind == MI_CTR_COL_DEC64 || kind == MI_CTR_COL_TIME) {
      if (oc >= 0 && oc < F) {
        a.keys[k * F_out + oc] = key;
      } else if (t.err) {
        atomicOr(t.err, MI_IDX_OUT_OF_RANGE);
      }
      if (kind == MI_CTR_COL_TIME && timed) {
        a.keys[k * F_out + F] = hour;
        a.keys[k * F_out + F + 1] = weekday;
        a.keys[k * F_out + F + 2] = weekday >= 5;
      }
    }
  }
}

// the checks the entry points share; fills everything of `t` but record / err_record / err.  A kept line has F separators
int set_up(Text &t, const uint8_t *text, int64_t nbytes, int64_t F, int32_t sep_byte, int32_t n_header, int64_t first_line_no,
           void *workspace) {
  if (nbytes < 0 || F < 0 || first_line_no < 0 || !workspace || (nbytes > 0 && !text)) return MI_ERR_INVALID_ARG;
  if (sep_byte < 1 || sep_byte > 255 || sep_byte == '\n' || sep_byte == '\r' || n_header < 0 || n_header > 1)
    return MI_ERR_INVALID_ARG;
  if (nbytes > (int64_t)INT32_MAX || F + 1 >= (1 << kColBits) || first_line_no > ((int64_t)1 << 46))
    return MI_ERR_UNSUPPORTED;                         // offsets stay below bit 31, (line, column) packs into 64 bits
  t.text = text;
  t.nbytes = nbytes;
  t.first_line_no = first_line_no;
  t.F = (int)F;
  t.sep = sep_byte;
  t.n_header = n_header;
  t.misalign = (int)(reinterpret_cast<uintptr_t>(text) & (kLaneBytes - 1));
  t.byte_tiles = (nbytes + 1 + t.misalign + kTileBytes - 1) / kTileBytes;
  t.final = 0;
  t.record = nullptr;
  t.err_record = nullptr;
  t.err = nullptr;
  lay_out(t, workspace, nbytes, t.F);
  return MI_OK;
}

// the six index launches over a chunk that set_up described
int launch_index(Text &t, int32_t is_final, int64_t *record, uint64_t *err_record, int *err, void *stream) {
  if (!record || !err_record) return MI_ERR_INVALID_ARG;
  t.final = is_final != 0;
  t.record = record;
  t.err_record = reinterpret_cast<unsigned long long *>(err_record);
  t.err = err;
  const int byte_grid = grid_for_tiles(t.byte_tiles), line_grid = grid_for_tiles(tiles_of(t.cap));
  MI_LAUNCH("ctr_text_count", k_text_count, byte_grid, kBlock, stream, t);
  MI_LAUNCH("ctr_text_scan_tiles", k_text_scan_tiles, 1, kBlock, stream, t);
  MI_LAUNCH("ctr_text_scatter", k_text_scatter, byte_grid, kBlock, stream, t);
  MI_LAUNCH("ctr_text_count_lines", k_text_count_lines, line_grid, kBlock, stream, t);
  MI_LAUNCH("ctr_text_scan_lines", k_text_scan_lines, 1, kBlock, stream, t);
  MI_LAUNCH("ctr_text_number_lines", k_text_number_lines, line_grid, kBlock, stream, t);
  return launch_status();
}

}  // namespace

extern "C" {

int64_t mi_ctr_text_workspace_bytes(int64_t nbytes, int32_t n_int, int32_t n_cat) {
  if (nbytes < 0 || nbytes > (int64_t)INT32_MAX || n_int < 0 || n_cat < 0) return 0;
  Text t;
  return lay_out(t, nullptr, nbytes, n_int + n_cat);
}

int mi_ctr_text_index(const uint8_t *text, int64_t nbytes, int32_t is_final, int32_t n_int, int32_t n_cat,
                      int64_t first_line_no, void *workspace, int64_t *record, uint64_t *err_record, int *err, void *stream) {
  if (n_int < 0 || n_cat < 0) return MI_ERR_INVALID_ARG;
  Text t;
  const int rc = set_up(t, text, nbytes, (int64_t)n_int + n_cat, '\t', 0, first_line_no, workspace);
  if (rc != MI_OK) return rc;
  return launch_index(t, is_final, record, err_record, err, stream);
}

int mi_ctr_text_parse(const uint8_t *text, int64_t nbytes, int32_t n_int, int32_t n_cat, const void *workspace, int64_t n_kept,
                      int64_t first_line_no, const int64_t *thresholds, int32_t n_thresholds, int64_t *keys_out,
                      uint8_t *labels_out, int64_t *line_no_out, uint64_t *err_record, int *err, void *stream) {
  if (n_int < 0 || n_cat < 0) return MI_ERR_INVALID_ARG;
  Parse a;
  const int rc = set_up(a.t, text, nbytes, (int64_t)n_int + n_cat, '\t', 0, first_line_no, const_cast<void *>(workspace));
  if (rc != MI_OK) return rc;
  if (n_kept < 0 || n_thresholds < 0 || !err_record || (n_thresholds > 0 && !thresholds)) return MI_ERR_INVALID_ARG;
  if (n_kept > a.t.kept_cap) return MI_ERR_INVALID_ARG;
  if (n_kept == 0) return MI_OK;
  if (!labels_out || !line_no_out || (a.t.F > 0 && !keys_out)) return MI_ERR_INVALID_ARG;
  a.t.err_record = reinterpret_cast<unsigned long long *>(err_record);
  a.t.err = err;
  a.n_kept = n_kept;
  a.n_int = n_int;
  a.thresholds = thresholds;
  a.n_thresholds = n_thresholds;
  a.keys = keys_out;
  a.labels = labels_out;
  a.line_no = line_no_out;
  const int64_t blocks = (n_kept * (a.t.F + 1) + kBlock - 1) / kBlock;
  MI_LAUNCH("ctr_text_parse", k_text_parse, (int)(blocks > kMaxGrid ? kMaxGrid : blocks), kBlock, stream, a);
  return launch_status();
}

int64_t mi_ctr_table_workspace_bytes(int64_t nbytes, int32_t n_cols) {
  if (nbytes < 0 || nbytes > (int64_t)INT32_MAX || n_cols < 1 || n_cols > kMaxCols) return 0;
  Text t;
  return lay_out(t, nullptr, nbytes, n_cols - 1);
}

int mi_ctr_table_index(const uint8_t *text, int64_t nbytes, int32_t is_final, int32_t sep_byte, int32_t n_cols,
                       int32_t n_header, int64_t first_line_no, void *workspace, int64_t *record, uint64_t *err_record,
                       int *err, void *stream) {
  if (n_cols < 1) return MI_ERR_INVALID_ARG;
  if (n_cols > kMaxCols) return MI_ERR_UNSUPPORTED;
  Text t;
  const int rc = set_up(t, text, nbytes, n_cols - 1, sep_byte, n_header, first_line_no, workspace);
  if (rc != MI_OK) return rc;
  return launch_index(t, is_final, record, err_record, err, stream);
}

int mi_ctr_table_parse(const uint8_t *text, int64_t nbytes, int32_t sep_byte, int32_t n_cols, const int32_t *spec,
                       int32_t derive_time, const void *workspace, int64_t n_kept, int64_t first_line_no, int64_t *keys_out,
                       uint8_t *labels_out, int64_t *line_no_out, uint64_t *err_record, int *err, void *stream) {
  if (n_cols < 1 || !spec) return MI_ERR_INVALID_ARG;
  if (n_cols > kMaxCols) return MI_ERR_UNSUPPORTED;
  TableParse a;
  // (the header count, which only moves line numbers here, is read from the workspace the index call left)
  const int rc = set_up(a.t, text, nbytes, n_cols - 1, sep_byte, 0, first_line_no, const_cast<void *>(workspace));
  if (rc != MI_OK) return rc;
  if (n_kept < 0 || !err_record || n_kept > a.t.kept_cap) return MI_ERR_INVALID_ARG;
  if (n_kept == 0) return MI_OK;
  if (!labels_out || !line_no_out || !keys_out) return MI_ERR_INVALID_ARG;
  a.t.err_record = reinterpret_cast<unsigned long long *>(err_record);
  a.t.err = err;
  a.n_kept = n_kept;
  a.spec = spec;
  a.derive_time = derive_time;
  a.keys = keys_out;
  a.labels = labels_out;
  a.line_no = line_no_out;
  const int64_t blocks = (n_kept * (int64_t)n_cols + kBlock - 1) / kBlock;
  MI_LAUNCH("ctr_table_parse", k_table_parse, (int)(blocks > kMaxGrid ? kMaxGrid : blocks), kBlock, stream, a);
  return launch_status();
}

}  // extern "C"
