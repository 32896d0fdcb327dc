// Metadata modalities of a STREAM that was encoded once (mused_amd/meta.py): the adjacency of window rows [s, e) from
// device-resident arrays that cover every row of the stream, written as the window-coordinate bitmask in one launch per
// modality.  Row validity, the records, the tag sets and their posting lists do not depend on the window, so nothing is
// gathered, re-numbered or uploaded per window and nothing is read on the host: the number of valid rows that caps k is
// read from vrank by the kernel.  The scores, the selection and the tie rule are those of mused_record_knn /
// mused_jaccard_knn -- the kernel is select_k_kernel of knn.hip with its windowed sources -- and invalid rows keep their
// window position, so the order among the valid rows (the tie rule) is that of the gathered rows of the host path.
// "username" needs no entry of its own: mused_group_mask on a slice of the stream's id array is the window's mask.
#include "common.h"
#include "internal.h"

using namespace mused;

static int window_ok(const char* who, int n_rows, int s, int e, int k, int mask_words, int cap) {
  MUSED_REQUIRE(n_rows >= 0 && s >= 0 && s <= e && e <= n_rows, "%s: rows [%d, %d) outside a stream of %d rows", who, s, e,
                n_rows);
  MUSED_REQUIRE(k >= 1, "%s: need k >= 1 (k=%d)", who, k);
  MUSED_REQUIRE(e - s <= cap, "%s: a window holds at most %d rows (got %d)", who, cap, e - s);
  MUSED_REQUIRE(mask_words >= cdiv(e - s, 64), "%s: mask_words=%d too small for %d rows", who, mask_words, e - s);
  return MUSED_OK;
}

extern "C" {

int mused_meta_window_records(const double* rec, const int* vrank, int n_rows, int kind, int s, int e, int k,
                              unsigned long long* out_mask, int mask_words, void* stream) {
  MUSED_REQUIRE(rec && vrank, "mused_meta_window_records: null argument");
  MUSED_REQUIRE(kind == 0 || kind == 1, "mused_meta_window_records: kind must be 0 (location) or 1 (time), got %d", kind);
  if (int rc = window_ok("mused_meta_window_records", n_rows, s, e, k, mask_words, select_max_fused_rows(false))) return rc;
  if (e == s) return MUSED_OK;
  MUSED_REQUIRE(out_mask, "mused_meta_window_records: null output");
  return select_window_records(rec, vrank, s, e, kind, k, out_mask, mask_words, (hipStream_t)stream);
}

int mused_meta_window_tags(const int* rowptr, const int* tag, const int* gpostptr, const int* gpostrow, const int* vrank,
                           int n_rows, int n_tags, int s, int e, int k, unsigned long long* out_mask, int mask_words,
                           void* stream) {
  MUSED_REQUIRE(rowptr && tag && gpostptr && gpostrow && vrank && n_tags >= 0, "mused_meta_window_tags: bad arguments (n_tags=%d)",
                n_tags);
  if (int rc = window_ok("mused_meta_window_tags", n_rows, s, e, k, mask_words, select_max_fused_rows(true))) return rc;
  if (e == s) return MUSED_OK;
  MUSED_REQUIRE(out_mask, "mused_meta_window_tags: null output");
  return select_window_tag_sets(rowptr, tag, gpostptr, gpostrow, vrank, s, e, k, out_mask, mask_words, (hipStream_t)stream);
}

}  // extern "C"
