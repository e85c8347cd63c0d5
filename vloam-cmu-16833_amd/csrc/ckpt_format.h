// Checkpoint of one sequence (vloam_checkpoint_save / vloam_checkpoint_load, c_api.h): the byte format and its parser.  Host only: no HIP, no
// handle.  A checkpoint is for the SAME BUILD of the library: the device structs it stores verbatim (LOState, MapState, FrameScalars, VoxelRec,
// vloam_sweep_record) are named by their sizes only, and a header whose sizes are not this build's is refused.
//
//   | CkptHeader | section 0 | section 1 | ... |     every section starts on an 8-byte boundary, in the order of the table, without gaps
//
// The header carries a magic, the format version, the struct sizes, the algorithmic parameters of the saving handle, the host-side counters
// of the sequence, the section table and a checksum over itself.  ckpt_parse validates ALL of it against the byte count it is given before
// the caller touches a device or a handle, and never reads outside [buf, buf + bytes).
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <string.h>

namespace vloam_ckpt {

constexpr char kMagic[8] = {'V', 'L', 'O', 'A', 'M', 'C', 'K', 'P'};
constexpr int kVersion = 1;

enum Section : int {
  kSecLoState = 0,   // 1 x LOState
  kSecMapState,      // 1 x MapState                          (none without mapping)
  kSecCubeCnt,       // 2 x kCubeNum ints                     (none without mapping)
  kSecMap,           // n_rec[0] corner records, then n_rec[1] surf records: the LIVE records of the two voxel tables as a dense stream of
                     // 32-byte VoxelRec {key, f32 sums, count, arrival stamp of a raw point}.  No slots, pend[], occupancy blocks, tombstones
                     // or deferred list: load rebuilds them.  Slot order of the saving table; load does not depend on the order.
  kSecScalars,       // 1 x FrameScalars of the last sweep    (none before the first sweep)
  kSecLessSharp,     // laserCloudCornerLast: n_less[0] float4
  kSecLessFlat,      // laserCloudSurfLast:   n_less[1] float4
  kSecStack0,        // the last mapped sweep's laserCloudCornerStack (vloam_get_features 7): n_stack[0] float4
  kSecStack1,        // ... laserCloudSurfStack (8): n_stack[1] float4
  kSecTraj,          // frames x 14 doubles
  kSecLog,           // frames x vloam_sweep_record, or none (the saving handle kept no log)
  kSecCount
};

enum StructSize : int { kSzLoState = 0, kSzMapState, kSzVoxelRec, kSzFrameScalars, kSzSweepRecord, kSzCubeInts /* 2 x kCubeNum */, kSzCount = 8 };

struct CkptSection { long long offset, bytes, count; };   // count records of bytes / count bytes each

struct CkptHeader {
  char magic[8];
  int version;
  int header_bytes;             // sizeof(CkptHeader)
  int struct_size[kSzCount];    // StructSize (unused entries 0)
  // algorithmic parameters: a handle that loads must have been created with the same
  int scan_line, mapping_skip_frame, detach_VO_LO, with_mapping;
  int stack_tier;               // 1: the saver had the large surf stack tier (arrival stamps of raw points keep 17 bits of stack index there)
  int pad0;
  float mapping_line_resolution, mapping_plane_resolution;
  double minimum_range;
  // the sequence
  int frames;                   // sweeps taken == trajectory rows
  int mapped;                   // mapped sweeps (mapping_skip_frame) == MapState::sweep_no
  unsigned ds_gen;              // scan-feature VoxelGrids enqueued
  int lo_launches;              // odometry association launches (parity of its queue counters)
  long long n_rec[2];           // live records of the corner / surf table
  long long n_blk[2];           // occupancy-block keys of the saver's tables (an upper bound of what load publishes)
  int n_deferred[2];            // raw voxels (load re-appends them)
  int n_less[2], n_stack[2];
  int n_sections;               // kSecCount
  int pad1;
  CkptSection sec[kSecCount];
  long long total_bytes;
  unsigned long long checksum;  // FNV-1a over the header with this field zero
};

struct CkptExpect { int struct_size[kSzCount]; };   // this build's sizes (the caller fills them: this header knows no device struct)

inline long long align8(long long x) { return (x + 7) & ~7ll; }
inline unsigned long long header_checksum(const CkptHeader& h) {
  CkptHeader c = h;
  c.checksum = 0;
  const unsigned char* p = reinterpret_cast<const unsigned char*>(&c);
  unsigned long long x = 1469598103934665603ull;
  for (size_t i = 0; i < sizeof(c); i++) { x ^= p[i]; x *= 1099511628211ull; }
  return x;
}
// bytes of one record of section s
inline long long section_elem(const CkptHeader& h, int s) {
  switch (s) {
    case kSecLoState: return h.struct_size[kSzLoState];
    case kSecMapState: return h.struct_size[kSzMapState];
    case kSecCubeCnt: return 4;
    case kSecMap: return h.struct_size[kSzVoxelRec];
    case kSecScalars: return h.struct_size[kSzFrameScalars];
    case kSecTraj: return 14 * 8;
    case kSecLog: return h.struct_size[kSzSweepRecord];
    default: return 16;   // float4 clouds
  }
}
// offsets, byte counts and total of a header whose counts are set
inline void layout(CkptHeader* h) {
  long long off = align8((long long)sizeof(CkptHeader));
  for (int s = 0; s < kSecCount; s++) {
    h->sec[s].offset = off;
    h->sec[s].bytes = h->sec[s].count * section_elem(*h, s);
    off = align8(off + h->sec[s].bytes);
  }
  h->total_bytes = off;
}

// Validates buf[0, bytes) and copies the header out.  false: err says why.  Nothing outside [buf, buf + bytes) is read.
inline bool ckpt_parse(const void* buf, long long bytes, const CkptExpect& ex, CkptHeader* out, char* err, size_t err_cap) {
  auto fail = [&](const char* what, long long a, long long b) { snprintf(err, err_cap, "checkpoint: %s (%lld, expected %lld)", what, a, b); return false; };
  if (!buf) return fail("null buffer", 0, 0);
  if (bytes < (long long)sizeof(CkptHeader)) return fail("shorter than its header", bytes, (long long)sizeof(CkptHeader));
  CkptHeader h;
  memcpy(&h, buf, sizeof(h));
  if (memcmp(h.magic, kMagic, sizeof(kMagic)) != 0) return fail("bad magic", 0, 0);
  if (h.version != kVersion) return fail("format version of another library", h.version, kVersion);
  if (h.header_bytes != (int)sizeof(CkptHeader)) return fail("header struct size of another build", h.header_bytes, (long long)sizeof(CkptHeader));
  for (int k = 0; k < kSzCount; k++)
    if (h.struct_size[k] != ex.struct_size[k]) return fail("device struct size of another build", h.struct_size[k], ex.struct_size[k]);
  if (h.checksum != header_checksum(h)) return fail("header checksum", 0, 0);
  if (h.total_bytes != bytes) return fail("total size", h.total_bytes, bytes);
  if (h.n_sections != kSecCount) return fail("section count", h.n_sections, kSecCount);
  if (h.scan_line != 16 && h.scan_line != 32 && h.scan_line != 64) return fail("scan_line", h.scan_line, 64);
  if (h.mapping_skip_frame < 1) return fail("mapping_skip_frame", h.mapping_skip_frame, 1);
  if ((h.with_mapping | 1) != 1 || (h.detach_VO_LO | 1) != 1 || (h.stack_tier | 1) != 1) return fail("a 0 / 1 parameter", h.with_mapping, 1);
  if (h.frames < 0) return fail("frame count", h.frames, 0);
  const long long mapped_most = h.with_mapping ? h.frames / h.mapping_skip_frame : 0;   // (a stage-wise caller may have left mapping calls out)
  if (h.mapped < 0 || h.mapped > mapped_most) return fail("mapped sweeps", h.mapped, mapped_most);
  for (int k = 0; k < 2; k++) {
    if (h.n_rec[k] < 0 || h.n_rec[k] > (1ll << 28)) return fail("record count of a table", h.n_rec[k], 0);
    if (h.n_blk[k] < 0 || h.n_blk[k] > (1ll << 28)) return fail("block keys of a table", h.n_blk[k], 0);
    if (h.n_deferred[k] < 0 || h.n_deferred[k] > h.n_rec[k]) return fail("raw voxels of a table", h.n_deferred[k], h.n_rec[k]);
    if (h.n_less[k] < 0 || h.n_stack[k] < 0) return fail("cloud size", h.n_less[k], 0);
  }
  const long long have = h.frames > 0 ? 1 : 0, m = h.with_mapping ? 1 : 0;
  const long long want[kSecCount] = {1, m, m * ex.struct_size[kSzCubeInts], h.n_rec[0] + h.n_rec[1], have, h.n_less[0], h.n_less[1], h.n_stack[0], h.n_stack[1],
                                     h.frames, h.sec[kSecLog].count == 0 ? 0 : h.frames};
  if (!h.with_mapping && (h.n_rec[0] | h.n_rec[1] | h.n_stack[0] | h.n_stack[1])) return fail("map of a sequence without mapping", h.n_rec[0] + h.n_rec[1], 0);
  if (!have && (h.n_less[0] | h.n_less[1])) return fail("clouds of a sequence without sweeps", h.n_less[0], 0);
  long long off = align8((long long)sizeof(CkptHeader));
  for (int s = 0; s < kSecCount; s++) {
    const CkptSection& S = h.sec[s];
    if (S.count != want[s]) return fail("records of a section", S.count, want[s]);
    if (S.bytes != S.count * section_elem(h, s)) return fail("length of a section", S.bytes, S.count * section_elem(h, s));   // (counts <= 2^29, records <= 2^20 bytes: no overflow)
    if (S.offset != off) return fail("offset of a section", S.offset, off);
    if (S.bytes > bytes - off) return fail("a section runs past the end", off + S.bytes, bytes);
    off = align8(off + S.bytes);
  }
  if (off != bytes) return fail("bytes behind the last section", bytes, off);
  *out = h;
  return true;
}

}  // namespace vloam_ckpt
