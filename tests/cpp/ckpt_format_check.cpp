// Stand-alone check of the checkpoint parser (csrc/ckpt_format.h, which is all this file includes of the library).  A valid small checkpoint is
// built in memory; the parser is then fed every truncation of it and every single-byte corruption of the header (which holds the section table),
// each from a heap buffer of exactly the size claimed, so that a read past the end is an AddressSanitizer error.  Built with
// -fsanitize=address,undefined and run on its own by tests/test_checkpoint_format.py.  Prints "OK <bytes> <cases>"; exit status 1 otherwise.
#include <stddef.h>
#include <initializer_list>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "ckpt_format.h"

using namespace vloam_ckpt;

static CkptExpect expect() {
  CkptExpect ex;
  memset(&ex, 0, sizeof(ex));
  ex.struct_size[kSzLoState] = 552; ex.struct_size[kSzMapState] = 224; ex.struct_size[kSzVoxelRec] = 32; ex.struct_size[kSzFrameScalars] = 1000;
  ex.struct_size[kSzSweepRecord] = 192; ex.struct_size[kSzCubeInts] = 2 * 4851;
  return ex;
}

static CkptHeader small_header(const CkptExpect& ex, int with_log) {
  CkptHeader h;
  memset(&h, 0, sizeof(h));
  memcpy(h.magic, kMagic, sizeof(kMagic));
  h.version = kVersion; h.header_bytes = (int)sizeof(CkptHeader);
  memcpy(h.struct_size, ex.struct_size, sizeof(ex.struct_size));
  h.scan_line = 16; h.mapping_skip_frame = 2; h.detach_VO_LO = 1; h.with_mapping = 1;
  h.mapping_line_resolution = 0.2f; h.mapping_plane_resolution = 0.4f; h.minimum_range = 0.3;
  h.frames = 5; h.mapped = 2; h.ds_gen = 2; h.lo_launches = 8;
  h.n_rec[0] = 7; h.n_rec[1] = 3; h.n_blk[0] = 4; h.n_blk[1] = 2; h.n_deferred[0] = 1; h.n_deferred[1] = 0;
  h.n_less[0] = 11; h.n_less[1] = 13; h.n_stack[0] = 5; h.n_stack[1] = 6;
  h.n_sections = kSecCount;
  const long long cnt[kSecCount] = {1, 1, ex.struct_size[kSzCubeInts], 10, 1, 11, 13, 5, 6, 5, with_log ? 5 : 0};
  for (int s = 0; s < kSecCount; s++) h.sec[s].count = cnt[s];
  layout(&h);
  h.checksum = header_checksum(h);
  return h;
}

// the parser on an exact-size heap copy of the first n bytes of src
static bool parse_copy(const unsigned char* src, long long n, const CkptExpect& ex, CkptHeader* out) {
  unsigned char* p = (unsigned char*)malloc(n > 0 ? (size_t)n : 1);
  if (n > 0) memcpy(p, src, (size_t)n);
  char err[256] = "";
  const bool ok = ckpt_parse(p, n, ex, out, err, sizeof(err));
  if (!ok && err[0] == 0) { fprintf(stderr, "a refusal without a message at %lld bytes\n", n); exit(1); }
  free(p);
  return ok;
}

int main() {
  const CkptExpect ex = expect();
  long long cases = 0, total = 0;
  for (int with_log = 0; with_log < 2; with_log++) {
    const CkptHeader h = small_header(ex, with_log);
    total = h.total_bytes;
    unsigned char* good = (unsigned char*)calloc(1, (size_t)total);
    memcpy(good, &h, sizeof(h));
    for (long long i = (long long)sizeof(h); i < total; i++) good[i] = (unsigned char)(i * 131 + 7);
    CkptHeader out;
    if (!parse_copy(good, total, ex, &out) || memcmp(&out, &h, sizeof(h)) != 0) { fprintf(stderr, "the valid checkpoint is refused\n"); return 1; }
    if (h.sec[kSecMap].bytes != 32 * (h.n_rec[0] + h.n_rec[1]) || h.sec[kSecLog].bytes != (with_log ? 5 * 192 : 0)) { fprintf(stderr, "section sizes\n"); return 1; }
    // every truncation, the empty buffer included
    for (long long n = 0; n < total; n++, cases++)
      if (parse_copy(good, n, ex, &out)) { fprintf(stderr, "a checkpoint cut to %lld of %lld bytes is accepted\n", n, total); return 1; }
    // a null buffer, and a longer buffer than the header says
    char err[256];
    if (ckpt_parse(nullptr, total, ex, &out, err, sizeof(err))) { fprintf(stderr, "null buffer accepted\n"); return 1; }
    {
      unsigned char* longer = (unsigned char*)calloc(1, (size_t)total + 8);
      memcpy(longer, good, (size_t)total);
      if (ckpt_parse(longer, total + 8, ex, &out, err, sizeof(err))) { fprintf(stderr, "trailing bytes accepted\n"); return 1; }
      free(longer);
    }
    // every single-byte corruption of the header (magic, version, sizes, parameters, counters, section table, total, checksum): three patterns per byte
    for (size_t i = 0; i < sizeof(CkptHeader); i++)
      for (unsigned char x : {(unsigned char)0x01, (unsigned char)0x80, (unsigned char)0xff}) {
        good[i] ^= x;
        cases++;
        if (parse_copy(good, total, ex, &out)) { fprintf(stderr, "header byte %zu ^ 0x%02x is accepted\n", i, x); return 1; }
        good[i] ^= x;
      }
    // ... and, with the checksum made right again, of the fields the parser must catch by itself: nothing may lead it outside the buffer
    for (size_t i = 0; i < sizeof(CkptHeader); i++) {
      CkptHeader c;
      good[i] ^= 0xff;
      memcpy(&c, good, sizeof(c));
      good[i] ^= 0xff;
      c.checksum = header_checksum(c);
      unsigned char* p = (unsigned char*)malloc((size_t)total);
      memcpy(p, good, (size_t)total);
      memcpy(p, &c, sizeof(c));
      const bool ok = ckpt_parse(p, total, ex, &out, err, sizeof(err));
      cases++;
      const size_t table = offsetof(CkptHeader, sec), parameters = offsetof(CkptHeader, scan_line);
      if (ok && (i < parameters || (i >= table && i < offsetof(CkptHeader, checksum)))) {   // (a changed parameter or counter can be another valid checkpoint)
        fprintf(stderr, "byte %zu of the magic / sizes / section table changed under a valid checksum is accepted\n", i); return 1;
      }
      if (ok) for (int s = 0; s < kSecCount; s++)
        if (out.sec[s].offset < (long long)sizeof(CkptHeader) || out.sec[s].bytes < 0 || out.sec[s].offset + out.sec[s].bytes > total) { fprintf(stderr, "accepted section %d leaves the buffer\n", s); return 1; }
      free(p);
    }
    // another build's struct size
    CkptExpect other = ex;
    other.struct_size[kSzMapState] += 8;
    if (parse_copy(good, total, other, &out)) { fprintf(stderr, "a struct size of another build is accepted\n"); return 1; }
    free(good);
  }
  printf("OK %lld %lld\n", total, cases);
  return 0;
}
