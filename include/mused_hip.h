/* libmused_hip -- C ABI of the MI355X (gfx950) hot path of mused.
 *
 * The reference (kelaendi/mused) has no FFI: its hot path sits behind two Python import lines,
 *   from matrix_operations import create_adjacency_matrix, fuse_matrices, perform_svd_reduction, ...   (main.py:5)
 *   from swfd import SeqBasedSWFD                                                                     (main.py:10)
 * This header is the drop-in boundary underneath those names: plain pointers and sizes, no torch
 * types.  Every pointer is a DEVICE pointer unless stated otherwise; `stream` is a hipStream_t;
 * outputs are caller-allocated; the library owns only the opaque handles.  Every function returns
 * 0 on success or a negative code (MUSED_ERR_*), the message is in mused_last_error().
 * No function synchronises with the host unless its comment says so.
 *
 * The Python host side that mirrors the reference's call surface on top of this ABI is
 * mused_amd/matrix_operations.py and mused_amd/swfd.py; INTEGRATION.md shows the binding.
 */
#ifndef MUSED_HIP_H
#define MUSED_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define MUSED_OK 0
#define MUSED_ERR_ARG -1
#define MUSED_ERR_HIP -2
#define MUSED_ERR_STATE -3
#define MUSED_ERR_UNSUPPORTED -4

/* element types of caller-provided row data */
#define MUSED_F32 0
#define MUSED_F64 1
#define MUSED_I64 2
/* mused_swfd_append* only: rows of a 0/1 matrix given as BITMASK rows (bit c of a row = element c; row pitch in
 * 64-bit words) -- the fused adjacency of matrix_operations.py:134-141 fed to the sketch (main.py:65-67) without
 * the dense W x W matrix ever being built */
#define MUSED_BITS 3

/* metric of the pairwise score */
#define MUSED_METRIC_L2 0     /* squared Euclidean, matrix_operations.py:112-119 (sklearn NearestNeighbors) */
#define MUSED_METRIC_COSINE 1 /* negated cosine similarity, matrix_operations.py:106-108 */

const char* mused_last_error(void);
int mused_version(void);
/* async device-to-device copy on `stream` */
int mused_memcpy_d2d(void* dst, const void* src, long bytes, void* stream);

/* ---- a1 / a2: similarity -> k nearest rows ------------------------------------------------- */

/* out[i] = sum_j X[i][j]^2 (fp64).  Row norms of main.py:61 and of sklearn's Euclidean / cosine kernels. */
int mused_row_sq_norms(const void* X, int dtype, long n, int d, long ld, double* out, void* stream);

/* S (n x n fp64, pitch n): metric L2: max(0, |x_i|^2 - 2 x_i.x_j + |x_j|^2); COSINE: -(x_i.x_j)/(|x_i||x_j|)
 * (zero norms -> 1).  norms: n-double workspace.  fp64 MFMA GEMM with fused epilogue. */
int mused_pairwise_scores(const void* X, int dtype, long n, int d, long ld, int metric, double* norms, double* S,
                          void* stream);

/* Per row of S the k smallest entries, ties to the smaller column.  out_idx (n x k int32, ascending
 * columns) and out_mask (n x mask_words uint64 bitmask, the row's own column cleared --
 * matrix_operations.py:128) may each be NULL. */
int mused_select_k_smallest(const double* S, long ld, int n, int k, int* out_idx, unsigned long long* out_mask,
                            int mask_words, void* stream);

/* Replaces NearestNeighbors(n_neighbors=k).fit(X).kneighbors(X) + the adjacency write loop
 * (matrix_operations.py:118-130), and cosine_similarity + argsort[:, :k] (:106-108), for dense rows.
 * ws_scores: n*n doubles, ws_norms: n doubles. */
int mused_knn_topk(const void* X, int dtype, long n, int d, long ld, int k, int metric, double* ws_scores,
                   double* ws_norms, int* out_idx, unsigned long long* out_mask, int mask_words, void* stream);

/* The same selection WITHOUT the n x n score matrix: scores are filtered against a per-row running threshold as they
 * leave the MFMA tiles (symmetric tile grid walked by cyclic tile distance, candidate lists of <= cap entries per row,
 * exact (score, column) selection between phases).  ws: mused_knn_fused_ws_bytes(n, cap) bytes, cap <= 1024.
 * *overflow_out (device int, written on `stream`) != 0: a row collected more than cap candidates, outputs INVALID:
 * redo that window with mused_knn_topk. */
long mused_knn_fused_ws_bytes(long n, int cap);
int mused_knn_fused(const void* X, int dtype, long n, int d, long ld, int k, int metric, void* ws, long ws_bytes, int cap,
                    int* out_idx, unsigned long long* out_mask, int mask_words, int* overflow_out, void* stream);

/* ---- a1, metadata modality types (/root/reference/matrix_operations.py:22-89) -----------------------
 * Scores for mused_select_k_smallest (smaller = closer), all n x n fp64 with pitch n.
 * mused_record_scores: rec = n x 2 fp64 records.  kind MUSED_REC_LOCATION: (latitude, longitude) in degrees ->
 *   haversine distance in km, the arithmetic of haversine_distance (:250-263) operation by operation; replaces
 *   NearestNeighbors(metric=haversine_distance).kneighbors (:29-30).  kind MUSED_REC_TIME: (datetaken, dateupload) ->
 *   |d datetaken| + |d dateupload| (:40-50); replaces the per-row argsort loop (:39-54).
 * mused_jaccard_scores: tag sets as CSR (rowptr[n + 1], tags[]: ids < n_tags, unique per row) plus the transposed
 *   posting lists (postptr[n_tags + 1], postrow[]); S[i][j] = -|Ti & Tj| / |Ti | Tj| (0 if either set is empty,
 *   jaccard_similarity :245-248), S[i][i] = +1 (the reference scores a row against itself with -1 and sorts
 *   descending, :87-88).  n <= 65536.
 * mused_group_mask: ids[n] (< 0: no user name) -> adjacency bitmask of "same id, other row" (:56-71, 123-130); any n. */
#define MUSED_REC_LOCATION 0
#define MUSED_REC_TIME 1
int mused_record_scores(const double* rec, int n, int kind, double* S, void* stream);
int mused_jaccard_scores(const int* rowptr, const int* tags, const int* postptr, const int* postrow, int n, int n_tags,
                         double* S, void* stream);
int mused_group_mask(const int* ids, int n, unsigned long long* out_mask, int mask_words, void* stream);
/* The same selections as mused_record_scores / mused_jaccard_scores followed by mused_select_k_smallest, WITHOUT the
 * n x n score matrix: the scores of a row are computed into LDS by the selection kernel itself (n <= 16384 records,
 * n <= 15000 tag sets).  Outputs as
 * mused_select_k_smallest (ties to the smaller row; own column cleared).  Either of out_idx and out_mask may be NULL, not
 * both; with a mask, mask_words >= ceil(n / 64) (words past the last column are written as zero).  Error, nothing
 * launched: both outputs NULL, a mask with a smaller mask_words, k < 1, k > n, n beyond the cap. */
int mused_record_knn(const double* rec, int n, int kind, int k, int* out_idx, unsigned long long* out_mask, int mask_words,
                     void* stream);
int mused_jaccard_knn(const int* rowptr, const int* tags, const int* postptr, const int* postrow, int n, int n_tags, int k,
                      int* out_idx, unsigned long long* out_mask, int mask_words, void* stream);

/* ---- a1, metadata types of a stream that was encoded ONCE (mused_amd/meta.py; csrc/meta_window.hip): the adjacency of
 * window rows [s, e) from arrays that cover all n_rows rows of the stream.  Enqueue-only; all arrays DEVICE, all integers
 * int32; nothing is read on the host and nothing is gathered, zero-filled or scattered around the call.
 * Stream: vrank[n_rows + 1] = prefix count of valid rows (row r is valid iff vrank[r + 1] != vrank[r]).
 *   mused_meta_window_records: rec = n_rows x 2 fp64 records, kind MUSED_REC_LOCATION / MUSED_REC_TIME.
 *   mused_meta_window_tags: rowptr[n_rows + 1], tag[] = tag sets as CSR over ALL rows with stream-global ids < n_tags
 *     (ascending inside a row, invalid rows empty); gpostptr[n_tags + 1], gpostrow[] = the rows that hold a tag,
 *     ascending: the part of a list inside [s, e) is one contiguous range, found by a binary search per list.
 * Output: the whole (e - s) x mask_words bitmask in WINDOW coordinates (mask_words >= ceil((e - s) / 64); words past the
 *   last column are written as zero).  An invalid row gets an empty row and is selected by no row; a valid row selects
 *   its min(k, n_valid) closest valid rows, n_valid = vrank[e] - vrank[s] read on the device, own bit cleared.  Scores,
 *   selection and tie rule (the smaller row) are those of mused_record_knn / mused_jaccard_knn on the gathered valid
 *   rows: invalid rows keep their position, so the order among the valid ones is the same.
 * e - s <= 16384 (records) / 15000 (tags); e == s is a successful no-op.  Error, nothing launched: s < 0, s > e,
 *   e > n_rows, kind other than 0 / 1, k < 1, mask_words too small, a window beyond the cap.
 * "username" needs no entry: mused_group_mask(uid + s, e - s, ...) on the stream's id array (< 0: no name). */
int mused_meta_window_records(const double* rec, const int* vrank, int n_rows, int kind, int s, int e, int k,
                              unsigned long long* out_mask, int mask_words, void* stream);
int mused_meta_window_tags(const int* rowptr, const int* tag, const int* gpostptr, const int* gpostrow, const int* vrank,
                           int n_rows, int n_tags, int s, int e, int k, unsigned long long* out_mask, int mask_words,
                           void* stream);

/* Batch scale (process_batch_data, main.py:132-167: the whole subset as one window, 150,000 rows by default): the same
 * selections for ANY n, with no n x n matrix and no global scratch.  One workgroup per row walks the columns in chunks of
 * at most `chunk` (0: the largest that fits, <= 16384) and keeps the row's k smallest (score, column) pairs in LDS;
 * ties to the smaller column.  Wherever mused_record_knn / mused_jaccard_knn apply the neighbour lists are identical.
 * out_idx (n x k int32, ascending columns) is required; out_mask (may be NULL; mask_words <= 8192) is built from it
 * (own column cleared).  k <= 1024.
 * mused_sparse_cosine_knn: the k_basis + 1 most similar rows of the "text" modality (matrix_operations.py:101-108) from
 *   the L2-normalised TF-IDF rows as CSR (rowptr[n + 1], terms[], vals[]: entries in the order scikit-learn stores them,
 *   NOT sorted) plus the per-term posting lists (postptr[n_terms + 1], postrow[] ascending, postval[]).  Similarity =
 *   sum over row i's entries in stored order of x_it * x_jt from 0, no FMA: SciPy's csr_matmat order behind
 *   cosine_similarity on sparse input, so the scores equal the reference's text_sim bit for bit; selected by the key
 *   0 - similarity (rows sharing no term score 0 and are taken in index order). */
int mused_record_knn_chunked(const double* rec, int n, int kind, int k, int chunk, int* out_idx,
                             unsigned long long* out_mask, int mask_words, void* stream);
int mused_jaccard_knn_chunked(const int* rowptr, const int* tags, const int* postptr, const int* postrow, int n, int n_tags,
                              int k, int chunk, int* out_idx, unsigned long long* out_mask, int mask_words, void* stream);
int mused_sparse_cosine_knn(const int* rowptr, const int* terms, const double* vals, const int* postptr, const int* postrow,
                            const double* postval, int n, int n_terms, int k, int chunk, int* out_idx,
                            unsigned long long* out_mask, int mask_words, void* stream);
/* Neighbour lists -> adjacency bitmask in window coordinates: list row r (idx: n_rows x k int32) becomes window row
 * row_map[r] with the bits row_map[idx[r][j]], the row's own column cleared (matrix_operations.py:123-130).  With a row
 * map every other row is empty (the mask is zero-filled first); row_map NULL: the identity, n_rows == n.
 * mask_words <= 8192 (n <= 524,288). */
int mused_lists_to_mask(const int* idx, int n_rows, int k, const int* row_map, int n, unsigned long long* out_mask,
                        int mask_words, void* stream);

/* ---- a2, "text": the TF-IDF of one window of a corpus that was tokenised once (matrix_operations.py:101-103:
 * TfidfVectorizer().fit_transform on the window's valid rows), csrc/tfidf.hip; specification: mused_amd/tfidf.py,
 * scikit-learn's indptr / indices / data bit for bit.  Enqueue-only; all arrays DEVICE, all integers int32.
 * Corpus (mused_amd/text.py; n_rows rows, n_terms global terms = ranks in the sorted vocabulary): rowptr[n_rows + 1],
 *   term[], cnt[] = CSR over all rows (invalid rows empty); pos[] = ordinal of the term's first occurrence in its
 *   document; vrank[n_rows + 1] = prefix count of valid rows, vrow[] = valid rank -> row; gpostptr[n_terms + 1],
 *   gpostrow[] (ascending rows), gpostent[] (the CSR entry of a posting) = term-major postings.
 *   max_row_terms: the longest row of the corpus, <= 1024 (one row is ranked in LDS).
 * Window: rows [s, e), n_docs = vrank[e] - vrank[s] >= 1 documents, nnz_w = rowptr[e] - rowptr[s] >= 1 entries (the
 *   caller has the host arrays and sizes the outputs from them); idf[j] = log((n_docs + 1) / (j + 1)) + 1 for
 *   j = 0 .. n_docs, computed on the host (the device never calls log).
 * Outputs: the window CSR in scikit-learn's STORED order (a row's entries ascend by the vocabulary's first-appearance
 *   numbering, not by column) -- out_rowptr[n_docs + 1], out_term[nnz_w] (global ids), out_col[nnz_w] (window column =
 *   rank among the present terms), out_val[nnz_w] (fit_transform's data), out_val2[nnz_w] (after normalize once more:
 *   what cosine_similarity multiplies) -- and the posting lists mused_sparse_cosine_knn reads with n_terms global terms:
 *   out_postptr[n_terms + 1] (absent terms: empty lists), out_postrow[nnz_w] (documents ascending), out_postval[nnz_w]
 *   (out_val2 of the entry).  info (4 int32) = {V_w present terms, flags, entries, 0}; flag 1: the window on the device
 *   is not the one the caller sized for (documents, entries or a row beyond max_row_terms) -- outputs invalid.
 * ws: mused_tfidf_ws_bytes(n_terms) bytes, 8-byte aligned (-1 for n_terms outside [1, 2^31)).
 * mused_tfidf_dense: the n_docs x n_cols fp64 matrix T.todense() (pitch ld, zero-filled here) from the window CSR. */
long mused_tfidf_ws_bytes(long n_terms);
int mused_tfidf_window(const int* rowptr, const int* term, const int* cnt, const int* pos, const int* vrank, const int* vrow,
                       const int* gpostptr, const int* gpostrow, const int* gpostent, int n_rows, int n_terms,
                       int max_row_terms, int s, int e, int n_docs, int nnz_w, const double* idf, int* out_rowptr,
                       int* out_term, int* out_col, double* out_val, double* out_val2, int* out_postptr, int* out_postrow,
                       double* out_postval, int* info, void* ws, long ws_bytes, void* stream);
int mused_tfidf_dense(const int* w_rowptr, const int* w_col, const double* w_val, int n_docs, int n_cols, double* out,
                      long ld, void* stream);

/* ---- a2, "text": the one tokenised pass itself (mused_amd/text.py: tokenise_on_device), csrc/tokenise.hip;
 * specification: mused_amd/tokens.py -- scikit-learn's default analyser on ASCII text as a rule on bytes (lower-case
 * 'A'..'Z'; every maximal run of [0-9A-Za-z_] of length >= 2 is a token; vocabulary in byte order).  All integers int32.
 * Input: buf (DEVICE, n_bytes in [1, 2^31), 16-byte aligned) = the strings of the n_docs valid rows, each followed by one
 *   separator byte that is no word byte; docptr_host (HOST, n_docs + 1 ints, read and checked at the call: from 0 to
 *   n_bytes, strictly ascending -- a document holds at least its separator -- and copied to the workspace on the stream).
 * Two calls, because the host sorts the V distinct tokens between them; both enqueue-only.  The workspace carries the
 * token spans (text order, from a prefix scan), the hash table and the lower-cased bytes from the first to the second.
 * mused_tokenise_scan: info (DEVICE, 4 ints) <- {T tokens, V distinct tokens, flags, tokens of the longest document};
 *   voc_start / voc_len (DEVICE, voc_cap ints each; n_bytes / 3 + 1 always suffices) <- byte span of one occurrence of
 *   every distinct token, in the order of the PROVISIONAL ids 0 .. V - 1 (table order: arbitrary, may differ from call
 *   to call).  table_slots: slots of the open-addressing table, 0 = the default 2 * (n_bytes / 3 + 1), at least twice
 *   T; any count in [1, 2^31) is accepted, and flag 2 is raised (nothing inserted, V = 0) when T exceeds it.
 *   max_doc_tokens in [1, 8192]: flag 1 when a document holds more tokens (the second call sorts a document in LDS).
 *   HOST READS after it: the 16 bytes of info, then voc_start[0 .. V) and voc_len[0 .. V).
 * mused_tokenise_build (same n_bytes, n_docs, table_slots, ws): n_tokens = T >= 1, n_terms = V in [1, 2^24),
 *   doc_tokens = info[3] in [1, 8192]; rank (DEVICE, V): provisional id -> rank in the sorted vocabulary; vrow (DEVICE,
 *   n_docs): document -> row.  Outputs (DEVICE): doc_rowptr[n_docs + 1] = CSR pointers over the DOCUMENTS (the host
 *   spreads them over all rows), term / cnt / pos [capacity T, nnz = doc_rowptr[n_docs] used] as TextCorpus documents
 *   them, gpostptr[V + 1], gpostrow / gpostent [capacity T] = the term-major postings (stable LSD radix sort of the
 *   entries by term).  info[2] |= 4: the workspace is not what the first call left (outputs invalid).
 *   HOST READS after it: doc_rowptr and info.
 * Nothing depends on scheduling: two runs give identical bytes in every output but voc_start / voc_len / rank.
 * ws: mused_tokenise_ws_bytes(n_bytes, n_docs, table_slots) bytes, 16-byte aligned (-1 for sizes out of range).
 * Bad arguments: MUSED_ERR_ARG, nothing enqueued, outputs untouched. */
long mused_tokenise_ws_bytes(long n_bytes, long n_docs, long table_slots);
int mused_tokenise_scan(const unsigned char* buf, long n_bytes, const int* docptr_host, long n_docs, long table_slots,
                        int max_doc_tokens, int* voc_start, int* voc_len, long voc_cap, int* info, void* ws, long ws_bytes,
                        void* stream);
int mused_tokenise_build(long n_bytes, long n_docs, long table_slots, int n_tokens, int n_terms, int doc_tokens,
                         const int* rank, const int* vrow, int* doc_rowptr, int* term, int* cnt, int* pos, int* gpostptr,
                         int* gpostrow, int* gpostent, int* info, void* ws, long ws_bytes, void* stream);

/* ---- a2, "text": the tokenised pass for text that is not pure ASCII (mused_amd/text.py: tokenise_codepoints_on_device),
 * csrc/tokenise.hip; specification: mused_amd/tokens.py, "code points" -- the same analyser as a rule on CODE POINTS: a
 * token is a maximal run of word code points of length >= 2 in code points, a run also ends behind a code point whose
 * lower case expands (U+0130), a token is the sequence of its lowered code points; vocabulary in code-point order.
 * The three entries mirror the byte entries above argument for argument; what differs:
 * Input: buf (DEVICE, n_cp uint32 code points, n_cp in [1, 2^30), 16-byte aligned), laid out as the byte buffer is, one
 *   element a code point, every U+03A3 already replaced by the host with its lower case in context (the final-sigma
 *   rule is not restated on the device); docptr_host in ELEMENTS.
 *   cls (DEVICE, n_cls uint32 in [128, 0x110000], read-only during the call, uploaded before it): the class table, entry
 *   c = lowered code point of c in bits 0..20 | bit 21 "word code point" | bit 22 "the run ends behind it".  The caller
 *   builds it from its own Unicode data (tokens.class_table()), so no Unicode version is compiled into the library.
 *   Code points below 128 take the rule of the byte entries, which entries 0..127 of a correct table equal; a code
 *   point >= n_cls is no word code point.
 * mused_tokenise_cp_scan: info, voc_start / voc_len (ELEMENT spans; capacity n_cp / 2 + 1 always suffices: two tokens
 *   may touch, "aİbİ" holds "ai" and "bi"), table_slots (0 = the default 2 * (n_cp / 2 + 1)), max_doc_tokens, flags
 *   and HOST READS as mused_tokenise_scan.  The host gathers the V spans from its own buffer through the same table.
 * mused_tokenise_cp_build: as mused_tokenise_build, n_cp in place of n_bytes, on the workspace the cp_scan call left.
 * ws: mused_tokenise_cp_ws_bytes(n_cp, n_docs, table_slots) bytes, 16-byte aligned (-1 for sizes out of range).
 * Bad arguments: MUSED_ERR_ARG, nothing enqueued, outputs untouched. */
long mused_tokenise_cp_ws_bytes(long n_cp, long n_docs, long table_slots);
int mused_tokenise_cp_scan(const unsigned* buf, long n_cp, const unsigned* cls, long n_cls, const int* docptr_host, long n_docs,
                           long table_slots, int max_doc_tokens, int* voc_start, int* voc_len, long voc_cap, int* info, void* ws,
                           long ws_bytes, void* stream);
int mused_tokenise_cp_build(long n_cp, long n_docs, long table_slots, int n_tokens, int n_terms, int doc_tokens, const int* rank,
                            const int* vrow, int* doc_rowptr, int* term, int* cnt, int* pos, int* gpostptr, int* gpostrow,
                            int* gpostent, int* info, void* ws, long ws_bytes, void* stream);

/* ---- a3 / a4: adjacency bitmasks -------------------------------------------------------------
 * An adjacency is n rows x words uint64 (words >= ceil(n/64)); bit j of row i <=> A[i][j] = 1. */

/* Replaces fuse_matrices (matrix_operations.py:134-141).  `masks`: HOST array of M device pointers. */
int mused_adj_fuse(const unsigned long long* const* masks, int M, int n, int words, unsigned long long* out,
                   void* stream);
/* Fusion by a truth table (not in the reference).  A subset s in [0, 2^M) has bit m set when modality m has the edge; the
 * table T is 256 bits (4 uint64, bit s of the table = bit s & 63 of word s >> 6).
 * out = T(masks): bit (i, j) of out = table bit s, s = sum_m bit_m(i, j) << m.  masks: HOST array of M (1 .. 8) device
 * pointers, n rows of `words` uint64 each; table: HOST, 4 uint64 (256 bits), bit 0 clear and no bit at or above 2^M set,
 * else MUSED_ERR_ARG.  ONE launch; every input word is read once, every output word written once; out may be any of the
 * inputs (a thread reads all of its inputs before it writes).  words >= ceil(n/64); all masks and out share the pitch.  T[0] = 0
 * keeps padding words and columns >= n clear for inputs that keep them clear.  Enqueue-only.  Bad arguments: MUSED_ERR_ARG,
 * nothing enqueued, out untouched. */
int mused_adj_fuse_table(const unsigned long long* const* masks, int M, const unsigned long long* table, int n, int words,
                         unsigned long long* out, void* stream);
/* The table of (weights, tau) built on the host, then the call above.  weights: HOST, M values finite and > 0, may be NULL = all
 * 1.0.  score(s) = the fp64 sum, from 0.0 and IN MODALITY ORDER, of w_m over the set bits of s (plain additions, nothing
 * reassociated); T[s] = 1 iff s != 0 and score(s) >= tau.  tau must be finite, > 0 and <= score(2^M - 1), else MUSED_ERR_ARG
 * with nothing enqueued: the table always accepts at least the full subset. */
int mused_adj_fuse_threshold(const unsigned long long* const* masks, const double* weights, int M, double tau, int n,
                             int words, unsigned long long* out, void* stream);
/* deg[n], rowptr[n+1] (exclusive scan), stats = {max degree, nnz}; max degree = R of main.py:61. */
int mused_adj_degrees(const unsigned long long* mask, int n, int words, int* deg, int* rowptr, int* stats,
                      void* stream);
int mused_adj_csr_fill(const unsigned long long* mask, int n, int words, const int* rowptr, int* colidx,
                       void* stream);
int mused_adj_transpose(const unsigned long long* mask, int n, int words, unsigned long long* out, void* stream);
/* dense n x n export (MUSED_F64: one modality, matrix_operations.py:135; MUSED_I64: fused, :138) */
int mused_adj_to_dense(const unsigned long long* mask, int n, int words, int dtype, void* out, void* stream);
/* dense import (nonzero -> edge); *nonbinary (device int, pre-zeroed) set if an entry is not 0/1 */
int mused_adj_from_dense(const void* dense, int dtype, int n, long ld, int words, unsigned long long* mask,
                         int* nonbinary, void* stream);
/* A value per entry of CSR lists, for mused_spmm_valued.  Weighted fusion S = sum_m w_m A_m of M (1 .. 8) bitmasks whose OR
 * gave the lists (`masks`, `weights`: HOST arrays; every weight finite and > 0): vals[e] = the fp64 sum from 0.0, in modality
 * order, of w_m over the modalities whose bit (i, colidx[e]) is set, e in rowptr[i] .. rowptr[i + 1].  transposed = 1: the
 * lists are those of the transposed mask, the bit read is (colidx[e], i).  Nothing is written behind rowptr[n].
 * Bad arguments (M, a null pointer, a weight <= 0 or not finite): MUSED_ERR_ARG, nothing enqueued. */
int mused_adj_csr_values(const unsigned long long* const* masks, const double* weights, int M, int n, int words,
                         const int* rowptr, const int* colidx, int transposed, double* vals, void* stream);
/* The same from a dense n x n matrix (MUSED_F32 / F64 / I64, row pitch ld) whose nonzeros gave the lists: vals[e] =
 * (double)dense[i][colidx[e]], or dense[colidx[e]][i] with transposed = 1.  *nonfinite (device int, pre-zeroed) is set when a
 * value is NaN or infinite. */
int mused_adj_csr_values_dense(const void* dense, int dtype, int n, long ld, const int* rowptr, const int* colidx,
                               int transposed, double* vals, int* nonfinite, void* stream);

/* ---- f3: hopping windows (step_window_ratio > 1, main.py:32) with reuse across consecutive windows --------------------
 * The same outputs as mused_knn_fused for the window whose row 0 is stream row lo_abs, computed from what the previous call
 * on the SAME workspace (the window n_new rows earlier) left behind: rows that stay keep their candidate lists minus the
 * columns that left; only the tiles involving one of the n_new entering rows (the LAST n_new rows of X) are evaluated:
 * 1 - (1 - n_new / n)^2 of the similarity work.  n_new = 0: from scratch (first window, or after a flag).  *flag_out
 * (device int) != 0: outputs INVALID (bit 0 a list overflowed, bit 1 a kept list no longer proves its row's k smallest) --
 * repeat with n_new = 0.  Bit-identical to mused_knn_fused on the same window. */
int mused_knn_fused_hop(const void* X, int dtype, long n, int d, long ld, int k, int metric, void* ws, long ws_bytes,
                        int cap, long lo_abs, int n_new, int* out_idx, unsigned long long* out_mask, int mask_words,
                        int* flag_out, void* stream);

/* ---- a8: randomized truncated SVD (perform_svd_reduction, matrix_operations.py:143-147) ------ */

int mused_rsvd_create(int n_max, int r_max, long nnz_cap, int sweeps, void** handle);
int mused_rsvd_destroy(void* handle);
/* buffer the fused adjacency bitmask (pitch ceil(n/64)) must be written to before mused_rsvd_reduce */
unsigned long long* mused_rsvd_mask_buffer(void* handle);
/* Q0 = np.random.RandomState(seed).normal(size=(n, r)) uploaded by the host (sklearn:utils/extmath.py:297) */
int mused_rsvd_set_q0(void* handle, const double* Q0, int n, int r, void* stream);
/* out_embed (n x n_comp) = X @ Vt.T, out_sigma (n_comp) = singular_values_, out_components (n x n_comp,
 * may be NULL) = Vt.T after svd_flip. */
int mused_rsvd_reduce(void* handle, int n, int n_comp, int r, int n_iter, double* out_embed, double* out_sigma,
                      double* out_components, void* stream);
/* mused_rsvd_reduce for the weighted fusion S = sum_m w_m A_m of M (1 .. 8) modality bitmasks (n rows of words =
 * ceil(n/64); `masks`, `weights`: HOST arrays, every weight finite and > 0, else MUSED_ERR_ARG).  The pattern is the OR of
 * the masks, which this call writes into the handle's mask buffer itself; the value of an edge is what
 * mused_adj_csr_values gives.  The handle allocates 16 * nnz_cap bytes for the values at its first valued call.  Masks and
 * weights may change from call to call. */
int mused_rsvd_reduce_weighted(void* handle, int n, int n_comp, int r, int n_iter,
                               const unsigned long long* const* masks, const double* weights, int M, int words,
                               double* out_embed, double* out_sigma, double* out_components, void* stream);
/* mused_rsvd_reduce for any square real matrix: dense n x n (MUSED_F32 / F64 / I64, row pitch ld, device).  Its nonzeros
 * are the pattern (built here, in the handle's mask buffer; at most nnz_cap < 2^31 of them), its entries as fp64 the values:
 * TruncatedSVD(n_comp, random_state -> Q0).fit_transform(dense).  A NaN, an infinity or a magnitude outside
 * [2^-200, 2^200] raises flags[1]; a matrix without a nonzero is not taken (the caller answers it: all zeros). */
int mused_rsvd_reduce_dense(void* handle, const void* dense, int dtype, long ld, int n, int n_comp, int r, int n_iter,
                            double* out_embed, double* out_sigma, double* out_components, void* stream);
/* device int[4] raised by mused_rsvd_reduce and its valued forms (flags[0] != 0: more than nnz_cap edges -> lists truncated,
 * result invalid but memory-safe; flags[1] != 0, valued calls only: a value was NaN or infinite (bit 0) or its magnitude outside
 * [2^-200, 2^200], beyond which the fp64 chain over- or underflows (bit 1) -- result invalid; flags[2]: weak Cholesky pivot, see mused_rsvd_set_mode; flags[3] != 0: the r x r eigensolve
 * gave up (work-queue timeout), result invalid); copy it on the same stream behind the call for a sync-free check */
const int* mused_rsvd_flags(void* handle);
/* How the eigenstep builds its bases.  0 (default): Cholesky-QR (Gram + Cholesky + triangular solve) with the
 * Householder chain recorded behind a weak-pivot flag: self-contained.  1: Cholesky-QR only -- flags[2] != 0 (third int of
 * mused_rsvd_flags) after a call means the result is INVALID (numerically rank-deficient panel): repeat the call on a
 * handle in mode 2.  2: the reference's chain (LU-normalised power iterations, Householder QR), launched kernel by kernel
 * without graph capture. */
int mused_rsvd_set_mode(void* handle, int mode);

/* BLOCKING: flags_out[0] != 0 -> more than nnz_cap edges; stats_out = {max out-deg, nnz, max in-deg, nnz} (HOST) */
int mused_rsvd_status(void* handle, int* flags_out, int* stats_out, void* stream);

/* building blocks of the eigenstep, exported for unit tests */
/* One Cholesky-QR pass of the eigenstep on the handle's scratch: Y, Q_out n x r (pitch r), r <= n, r <= 286, handle not in
 * mode 2.  G_out / L_out: Gram (rb x rb) and packed lower factor (rb (rb + 1) / 2) of the last block factorised -- rb = r
 * for r <= 143, else the second block, rb = r - r / 2.  weak_out: one int, the weak-pivot word.  All device pointers. */
int mused_rsvd_cholqr(void* handle, const double* Y, int n, int r, double* Q_out, double* G_out, double* L_out,
                      int* weak_out, void* stream);
/* The eigenstep's selection tail on eigenpairs of the caller: evals (en), U (en x en, columns), en = (r_max + 1) & ~1;
 * Bt n x r (pitch r).  V_out (n x n_comp) = Bt U[:, order] S^-1 after svd_flip, sigma_out (n_comp) descending. */
int mused_rsvd_select(void* handle, const double* evals, const double* U, const double* Bt, int n, int r, int n_comp,
                      double* V_out, double* sigma_out, void* stream);
int mused_spmm_binary(const int* rowptr, const int* colidx, int n, const double* Q, long ldq, int r, double* Y,
                      long ldy, void* stream);
/* Y = S Q for lists with one fp64 value per entry (mused_adj_csr_values): every Y[i][c] is accumulated by one lane over row
 * i's list, in list order, from 0.0, acc = acc + (vals[e] * Q[colidx[e]][c]) with the product rounded before the add (no
 * fused multiply-add).  With every value 1.0 the result is mused_spmm_binary's, bit for bit.  The shape rule and
 * mused_spmm_force_path / MUSED_SPMM apply as for mused_spmm_binary (a forced kernel: mused_spmm_binary_path); unforced, the
 * wide kernel runs wherever the shape can take it.  Both kernels give the same bits. */
int mused_spmm_valued(const int* rowptr, const int* colidx, const double* vals, int n, const double* Q, long ldq, int r,
                      double* Y, long ldy, void* stream);
/* Which kernel mused_spmm_binary runs for these arguments: 0 rows (any shape), 1 wide (r even, rows of Q 16-byte aligned).
 * q_align / y_align: the base pointers of Q and Y modulo 16 bytes. */
int mused_spmm_binary_path(int n, int r, long ldq, long ldy, int q_align, int y_align);
/* Test-facing: force that kernel wherever the shape can take it, as MUSED_SPMM=rows|wide does; -1: the default.
 * An eigenstep handle records its kernels when it first runs a shape. */
int mused_spmm_force_path(int path);
/* ws_int: n + ceil(n/16) ints, ws_f64: 4 * (r + n) doubles */
int mused_lu_permute_l(double* Y, int n, int r, long ld, int* ws_int, double* ws_f64, void* stream);
/* Diagnostics, no device needed.  mused_lu_mode: the LU variant MUSED_LU_MODE / MUSED_LU_BLOCKED ask for, read once per
 * process: 0 column-at-a-time, 1 blocked panels (the default), 2 one launch per column.  mused_lu_path: the variant
 * mused_lu_permute_l runs for an n x r panel (the blocked panels hold at most 10,240 rows; above that the column-at-a-time
 * kernels run); -1 for a shape it rejects.  All three variants give the same bits. */
int mused_lu_mode(void);
int mused_lu_path(int n, int r);
/* ws_f64: r + ceil(n/512) * r + 2 n doubles; n >= r */
int mused_qr_economic(double* Y, int n, int r, long ldy, double* Q, long ldq, double* ws_f64, void* stream);
/* BLOCKING (creates/destroys its plan): eigen-decomposition of `batch` symmetric n x n matrices, n even */
int mused_syevj_batched(const double* G, int n, int batch, int sweeps, double* evals, double* V, void* stream);
int mused_gemm_f64(int a_kc, int b_kc, const double* A, long lda, const double* B, long ldb, double* C, long ldc,
                   int M, int N, int K, double alpha, void* stream);
int mused_gemm_f64_batched(int a_kc, int b_kc, const double* A, long lda, long strideA, const double* B, long ldb,
                           long strideB, double* C, long ldc, long strideC, int M, int N, int K, int batch,
                           double alpha, void* stream);
/* Diagnostic entries for the launch modes the library uses inside (unit tests).  A == B with equal layouts, leading
 * dimensions and strides and M == N selects the symmetric launch (tiles on or above the diagonal, mirrored stores) in
 * every GEMM entry, as inside the library.
 * mused_gemm_f64_batched_rep: mused_gemm_f64_batched, but entry z is computed only if rep[z] == z (rep: batch device
 *   ints; the C of the other entries is not written).
 * mused_gemm_f64_splitk: partial (nsplit x M x N, pitch N) = the products over k in [s kchunk, (s + 1) kchunk), then C (M x N,
 *   pitch N, alpha = 1) = their sum in split order.  kchunk > 0 a multiple of 16, nsplit >= 1, kchunk * nsplit >= K.
 * mused_gemm_f64_batched_splitk: the same per batch entry (partial: batch x nsplit x M x N, C: batch x M x N), entries with
 *   rep[z] != z skipped in both steps (rep may be NULL).
 * mused_kmeans_assign_rows: the rows per LDS sub-tile of the E/M-step kernel mused_kmeans_lloyd launches for (d, k): 64,
 *   32 or 16 (the largest whose LDS need fits), 0 = the row-per-thread kernel (what MUSED_KMEANS_ASSIGN=p forces); -1
 *   where mused_kmeans_lloyd rejects (d, k). */
int mused_gemm_f64_batched_rep(int a_kc, int b_kc, const double* A, long lda, long strideA, const double* B, long ldb,
                               long strideB, double* C, long ldc, long strideC, int M, int N, int K, int batch,
                               double alpha, const int* rep, void* stream);
int mused_gemm_f64_splitk(int a_kc, int b_kc, const double* A, long lda, const double* B, long ldb, double* partial,
                          double* C, int M, int N, int K, int kchunk, int nsplit, void* stream);
int mused_gemm_f64_batched_splitk(int a_kc, int b_kc, const double* A, long lda, long strideA, const double* B, long ldb,
                                  long strideB, double* partial, double* C, int M, int N, int K, int batch, int kchunk,
                                  int nsplit, const int* rep, void* stream);
int mused_kmeans_assign_rows(int d, int k);

/* ---- a10 / f2: the Lloyd iterations of perform_clustering (matrix_operations.py:149-153, sklearn KMeans) ------------
 * The seeds come from mused_kmeans_seed below (or from scikit-learn's own routine on the host); E / M steps and
 * the stopping rule of sklearn's _kmeans_single_lloyd run here in fp64 with fixed-order sums.  X: n x d fp64 embedding
 * (pitch ld), mean: its d column means, centers: k x d seeds of the CENTRED rows (in/out), tol = mean(var(X, 0)) * 1e-4.
 * labels_out: n int32 (device); info_out (HOST, 4 ints) = {iterations, 1 strict / 2 tol / 0 max_iter, empty-cluster flag
 * (result invalid: use scikit-learn for that window), 0}.  BLOCKING.  k * d <= 8192. */
long mused_kmeans_ws_bytes(int n, int d, int k);
int mused_kmeans_lloyd(const double* X, long ld, int n, int d, int k, const double* mean, double* centers, double tol,
                       int max_iter, int* labels_out, int* info_out, void* ws, long ws_bytes, void* stream);
/* mused_kmeans_lloyd_wide: the same arguments and contract for any k <= 1024, d <= 512, k <= n (the limits of
 *   mused_kmeans_seed and mused_kmeans_assign): the centres stream through LDS in tiles, the M-step partials take a tile
 *   of columns per workgroup and the centre sums are spread over workgroups, every sum in mused_kmeans_lloyd's order, so
 *   labels, info and the BITS of the centres equal mused_kmeans_lloyd's wherever both accept the shape.  BLOCKING.
 *   ws: mused_kmeans_wide_ws_bytes(n, d, k) bytes (-1 for a rejected shape).
 * mused_kmeans_wide_tiles: out[0..2] = {rows per tile, centres per tile of the E step (LDS 8 (out[0] + out[1]) (d + 1)
 *   bytes), columns per tile of the M-step partials (LDS 8 k out[2] + 1040 bytes)} for (d, k); needs no device. */
long mused_kmeans_wide_ws_bytes(int n, int d, int k);
int mused_kmeans_lloyd_wide(const double* X, long ld, int n, int d, int k, const double* mean, double* centers, double tol,
                            int max_iter, int* labels_out, int* info_out, void* ws, long ws_bytes, void* stream);
int mused_kmeans_wide_tiles(int d, int k, int* out);

/* ---- what KMeans.fit does before the Lloyd iterations (csrc/kmeanspp.hip).  Both enqueue-only, fp64, fixed-order sums.
 * mused_kmeans_moments: mean_out (d, device) = X.mean(axis=0) bit for bit (rows added in row order, / n); tol_out (1,
 *   device) = mean(var(X, 0)) * 1e-4 with NumPy's steps for the variances (squares rounded, added in row order, / n).
 * mused_kmeans_seed: sklearn `_kmeans_plusplus` on the rows X - mean with the generator's draws made up front on the host:
 *   first = the first centre's row, U = (k - 1) x trials uniforms (DEVICE), trials = 2 + int(log(k)) <= 8.  centers_out:
 *   k x d centred rows (the layout mused_kmeans_lloyd takes), indices_out: k int32 row indices, info_dev (2 int32, DEVICE) =
 *   {ambiguity flag, centres chosen}.  The sums are not taken in scikit-learn's order; the flag is raised when a search or
 *   the choice among the candidates was decided within 2 E, E = 4 (d + 8) 2^-52 (sum |x_i|^2 + n max |x_i|^2): seed that
 *   window with scikit-learn then.  k <= 1024, d <= 512, k <= n.  ws: mused_kmeans_seed_ws_bytes(n, d, k) bytes; its third
 *   block of n doubles (after the n x d centred rows and the n row norms, each block rounded up to 256 bytes) holds
 *   closest_dist_sq when the call has run. */
int mused_kmeans_moments(const double* X, long ld, int n, int d, double* mean_out, double* tol_out, void* stream);
long mused_kmeans_seed_ws_bytes(int n, int d, int k);
int mused_kmeans_seed(const double* X, long ld, int n, int d, int k, const double* mean, int first, const double* U, int trials,
                      double* centers_out, int* indices_out, int* info_dev, void* ws, long ws_bytes, void* stream);

/* ---- sSVDMC_mini: MiniBatchKMeans(n_clusters_total, random_state=seed, batch_size=W).partial_fit(X).predict(X) --------
 * (main.py:82-86; sklearn 1.7 cluster/_kmeans.py).  The arithmetic only: the RandomState stays on the host (k-means++ on the
 * first batch, _random_reassign, the trim and rows of the reassignment, mused_amd/cluster.py), which keeps a copy of the
 * k counts.  X: n x d fp64, pitch ld, UNCENTRED; centers: k x d fp64 (pitch d); counts: k fp64.  k <= 1024, d <= 512, no
 * k * d bound.  ws: mused_mbkm_ws_bytes(n, d, k) bytes.  Enqueue-only.
 * mused_mbkm_step: labels (n int32, out) = the E step of _mini_batch_step (:1624, _labels_inertia; csq - 2 x.c with the
 *   fma-chain dot of mused_kmeans_lloyd, first minimum on ties), then _minibatch_update_dense (:1632-1640,
 *   _k_means_minibatch.pyx update_center_dense): per cluster with rows c <- c * counts, + rows in sample order,
 *   counts += rows, c *= 1 / counts -- bit-identical to scikit-learn's centres and counts wherever the labels agree.
 * mused_mbkm_reassign: centers[dst_centers[i]] <- X[src_rows[i]] for i < m, counts <- new_counts (k fp64): the device half
 *   of :1643-1673 (centers_new[to_reassign] = X[new_centers]; weight_sums[to_reassign] = min(...)).  Pairs outside
 *   [0, n) x [0, k) are skipped.  m <= k.
 * mused_kmeans_assign: labels (n int32) of X against the centres, the same E step (predict, :1066; labels_ after
 *   partial_fit, :2293). */
long mused_mbkm_ws_bytes(int n, int d, int k);
int mused_mbkm_step(const double* X, long ld, int n, int d, int k, double* centers, double* counts, int* labels, void* ws,
                    long ws_bytes, void* stream);
int mused_mbkm_reassign(const double* X, long ld, int n, int d, int k, const int* src_rows, const int* dst_centers, int m,
                        const double* new_counts, double* centers, double* counts, void* stream);
int mused_kmeans_assign(const double* X, long ld, int n, int d, int k, const double* centers, int* labels, void* ws,
                        long ws_bytes, void* stream);

/* ---- sSVDMC_pot: the label chain match_clusters(prev, new, "pot", min_overlap) (matrix_operations.py:155-210) ---------
 * with ot.sinkhorn(a, b, M, reg=0.1) written out (Sinkhorn-Knopp, 1000 iterations at most, stopThr 1e-9; the specification
 * is mused_amd/sinkhorn.py -- POT itself is not available: specified, unpinned).  csrc/match.hip, ONE launch of one
 * workgroup for the whole chain, enqueue-only.
 * raw: K_windows x W int32 labels (DEVICE); matched_out: K_windows x W int32; for t = 0 .. K_windows - 1
 *   matched_t = match(matched_{t-1}, raw_t), window 0 against prev0 (W int32, DEVICE) or copied through when prev0 is NULL.
 * info_out (DEVICE, 8 int32 per window) = {P, N, iterations run, feasible, flag word, the smallest relative distance of a
 *   plan entry from the selection threshold (float32 bits), 1 when matched_t was written, 0}.
 * Flag word: 1 a plan entry within delta of 0.5 max(plan), 2 an error check within delta' of stopThr (the sums are not
 *   taken in NumPy's order: a decision within rounding is not made here), 4 a label outside [0, 1024), 8 P or N beyond 256.
 *   The chain ENDS at the first flagged window: that window and the ones behind it are not written (info word 6 = 0);
 *   match it on the host and call again from the next window with its labels as prev0.
 * plan_out (DEVICE, may be NULL; diagnostic): K_windows x 65536 doubles, window t's P x N plan at t * 65536, pitch N.
 * ws: mused_match_pot_ws_bytes() bytes. */
long mused_match_pot_ws_bytes(void);
int mused_match_pot_chain(const int* raw, int K_windows, int W, const int* prev0, int min_overlap, int* matched_out,
                          int* info_out, double* plan_out, void* ws, long ws_bytes, void* stream);

/* ---- sSVDMC, sSVDMC_hung, SWFDMC, sSVDMC_mini: the label chain match_clusters(prev, new, "hungarian", min_overlap) -----
 * (matrix_operations.py:155-185) with scipy.optimize.linear_sum_assignment written out (shortest augmenting paths, SciPy's
 * scan order and tie rule, integer arithmetic: the specification is mused_amd/hungarian.py, pinned to SciPy by the tests).
 * csrc/match_hung.hip, ONE launch of one workgroup for the whole chain, enqueue-only.
 * raw, prev0, matched_out: as for mused_match_pot_chain.
 * info_out (DEVICE, 8 int32 per window) = {P, N, Dijkstra steps of the solver, feasible (every row and column of the cost
 *   matrix keeps a finite entry; when 0 the window passes through unmatched), flag word, 0, 1 when matched_t was written, 0}.
 * Flag word: 4 a label outside [0, 1024), 8 P or N beyond 256, 16 the feasibility test passed but no complete assignment
 *   exists (SciPy raises ValueError there).  The chain ENDS at the first flagged window: that window and the ones behind
 *   it are not written (info word 6 = 0); match it on the host and call again from the next window with its labels as prev0.
 * assign_out (DEVICE, may be NULL; diagnostic): K_windows x 256 int32, the column assigned to each row of window t's P x N
 *   cost matrix at t * 256, or -1.
 * ws: mused_match_hung_ws_bytes() bytes. */
long mused_match_hung_ws_bytes(void);
int mused_match_hung_chain(const int* raw, int K_windows, int W, const int* prev0, int min_overlap, int* matched_out,
                           int* info_out, int* assign_out, void* ws, long ws_bytes, void* stream);

/* ---- The same label chain for density labels: ANY int32 label value (the noise label -1, INT32_MIN and INT32_MAX
 * included) and up to 4096 distinct labels a side -- what DBSCAN_incr produces and the entry above flags 4 or 8.
 * csrc/match_wide.hip; the specification is hungarian.match_labels (mused_amd/hungarian.py).  Seven launches per window,
 * enqueue-only: no host read or wait inside the call.  Labels are 32 bits: 64-bit labels must be narrowed by the CALLER,
 * and a value that does not fit int32 must not be sent here.
 * raw, prev0, matched_out: as for mused_match_hung_chain.  W in [1, 2^20] (the solver's 64-bit key is proved for overlap
 *   counts up to 2^20 and 4096 positions; any other W is MUSED_ERR_ARG), K_windows * W < 2^31.
 * info_out (DEVICE, 8 int32 per window), as above = {P, N, Dijkstra steps, feasible, flag word, 0, 1 when matched_t was
 *   written, 0}.
 * Flag word: 8 P or N beyond 4096 (that side's word then holds 4097), 16 the feasibility test passed but no complete
 *   assignment exists (SciPy raises ValueError there), 32 the solver would take more than max_steps Dijkstra steps
 *   (max_steps = 0: 32 min(P, N); ordinary label pairs take about 2 min(P, N), the worst case is min(P, N)^2 -- a guard
 *   for a shared device, not a tuning knob).  There is no flag 4: every int32 is a label.  The chain ENDS at the first
 *   flagged window as above.
 * assign_out (DEVICE, may be NULL; diagnostic): K_windows x 4096 int32, the column of each row of the P x N matrix or -1.
 * ws: mused_match_hung_wide_ws_bytes(W) bytes, 256-byte aligned:
 *   256 + 8 * 2 * 16384 + 4 * 6 * 4096 + align256(4 W) + align256(4 min(W, 4096)^2)
 *   (control block, two hash sets, value / mark / map tables, one rank per row, the dense overlap counts: 352.25 KiB + 4 W
 *   + 4 min(W, 4096)^2, at most 68.4 MiB); -1 for W outside [1, 2^20]. */
long mused_match_hung_wide_ws_bytes(int W);
int mused_match_hung_wide_chain(const int* raw, int K_windows, int W, const int* prev0, int min_overlap, long max_steps,
                                int* matched_out, int* info_out, int* assign_out, void* ws, long ws_bytes, void* stream);

/* ---- DBSCAN_batch: perform_dbscan_clustering (matrix_operations.py:235-238, sklearn DBSCAN(eps, min_samples,
 * metric="euclidean").fit_predict) on fp64 rows, csrc/dbscan.hip.  scikit-learn's index-order search in closed form
 * (specification: mused_amd/dbscan.py): core rows have >= min_samples rows within eps (themselves included), clusters are the
 * connected components of the core rows numbered by ascending smallest core index, another row takes the smallest label
 * among its core neighbours or -1.  Three passes over the fp64 MFMA distance tiles (count, union-find, border rows) and
 * O(n) workspace: no n x n array, neighbour list or bitmask.  Enqueue-only.
 * X: n x d fp64 (pitch ld), n <= 2^19 (the tile grid of one launch).  labels_out: n int32 (DEVICE).  info_out (DEVICE, 4 int32) = {flags, clusters, core
 *   rows, 0}.  Flags: 1 some pair i != j has | d2 - eps^2 | <= 2 (d + 8) 2^-52 (|x_i|^2 + |x_j|^2) + 4 ulp(eps^2), the bound
 *   within which two ways of evaluating d2 can disagree; 2 a row is not finite.  With either flag the labels are NOT
 *   scikit-learn's: call it on the host (it raises on non-finite input).
 * ws: mused_dbscan_ws_bytes(n) bytes (24 n + 4 ceil(n / 128) and alignment; -1 for n outside [1, 2^19]). */
long mused_dbscan_ws_bytes(long n);
int mused_dbscan(const double* X, long n, int d, long ld, double eps, int min_samples, int* labels_out, int* info_out,
                 void* ws, long ws_bytes, void* stream);

/* ---- DBSCAN_incr: incremental DBSCAN under insertions (main.py:87-91: IncrementalDBSCAN(eps, min_pts), insert per window),
 * csrc/dbscan_incr.hip.  After every insert the labels of ALL rows inserted so far equal sklearn DBSCAN(eps, min_samples,
 * metric="euclidean").fit_predict(those rows), numbering included (specification: mused_amd/dbscan_incr.py; pinned to
 * scikit-learn's refit, NOT to the `incdbscan` package).  An insert runs the fp64 MFMA distance tiles of (new rows) x (all
 * rows) for the counts, (rows that turned core) x (all rows) for the union-find, and for min_samples >= 3 (core rows whose
 * root moved) x (all rows) and (new rows) x (all rows) for the border rows; never all x all, no n x n array or neighbour list.
 * NOT enqueue-only: the call reads the dirty counts between its phases and returns after the stream has finished.
 * X: ALL n0 + w rows, fp64 (pitch ld), the w new rows in place behind the n0 old ones; n0 + w <= 2^19.
 * nrm (fp64), count, parent, best (int32): the caller's state arrays, n0 + w entries at least, kept from insert to insert
 *   (what they hold for the n0 old rows is read; n0 = 0 starts a stream: nothing is read).  Rows may move to larger arrays
 *   between inserts as long as their contents move with them.
 * chunk: rows per staging panel, a multiple of 128 in [128, 65536].
 * labels_out: n0 + w int32 (DEVICE), -1 = noise.  info_out (HOST, 6 int32) = {flags, clusters, core rows, dirty rows,
 *   rows that turned core, core rows whose root moved}; dirty rows is the sum of the last two.  Flags as mused_dbscan: 1
 *   some pair of this insert lies within tau of eps^2, 2 a new row is not finite.  With either flag the call stops behind
 *   the counting pass: labels_out is NOT written and the state is spent (refit on the host, start a new state).
 * ws: mused_dbscan_incr_ws_bytes(capacity, d, chunk) bytes for any capacity >= n0 + w (16 capacity + 8 ceil(capacity / 128)
 *   + 8 chunk (d rounded up to even) and alignment; -1 for capacity outside [1, 2^19] or a bad d or chunk).  Scratch only:
 *   it carries nothing from insert to insert.  Outside these limits the call returns an error and writes nothing. */
long mused_dbscan_incr_ws_bytes(long capacity, int d, long chunk);
int mused_dbscan_incr_insert(const double* X, long ld, int d, double* nrm, int* count, int* parent, int* best, long n0, long w,
                             double eps, int min_samples, long chunk, int* labels_out, int* info_out, void* ws, long ws_bytes,
                             void* stream);

/* ---- DBSCAN_incr over a sliding window: the m OLDEST of the n rows held are deleted, csrc/dbscan_incr.hip.  Afterwards the
 * labels of the n - m rows still held equal sklearn DBSCAN(eps, min_samples, metric="euclidean").fit_predict(those rows, in
 * their order), numbering included, after any sequence of inserts and deletes (specification: mused_amd/dbscan_incr.py,
 * `delete_oldest`; pinned to scikit-learn's refit).  A delete runs the fp64 MFMA distance tiles of (deleted rows) x (survivors)
 * for the counts, (surviving core rows of the components that lost a core row) x (survivors) to rebuild those components, and for
 * min_samples >= 3 (non-core rows whose cluster may have changed) x (survivors); components the delete does not touch cost
 * nothing.  There is no rounding flag: every pair was tested when the later of its rows was inserted.
 * NOT enqueue-only: the call reads the two list lengths between its phases and returns after the stream has finished.
 * X: the n rows held, fp64 (pitch ld), n <= 2^19; they are NOT modified.  Afterwards the caller's rows start at X + m * ld.
 * nrm, count, parent, best: the state arrays of mused_dbscan_incr_insert over the n rows; on return entries [0, n - m) describe
 *   the survivors in the new numbering (survivor i has become i - m).  They are written shifted into the workspace and copied
 *   back, so no entry is read after it has been overwritten.  m == n leaves the empty state (the next insert has n0 = 0).
 * m: 1 <= m <= n.  chunk: rows per staging panel, a multiple of 128 in [128, 65536].
 * labels_out: n - m int32 (DEVICE), -1 = noise.  info_out (HOST, 6 int32) = {flags (always 0), clusters, core rows, rows that
 *   lost core status, rows whose components were rebuilt (|R|), non-core rows taken against the core rows again (|B|)}.
 * ws: mused_dbscan_incr_delete_ws_bytes(capacity, d, chunk) bytes for any capacity >= n (44 capacity + 4 ceil(capacity / 128)
 *   + 8 chunk (d rounded up to even) and alignment; -1 for capacity outside [1, 2^19] or a bad d or chunk).  Scratch only.
 *   Outside these limits (m outside [1, n], a short workspace, a bad chunk or d) the call returns an error and writes nothing. */
long mused_dbscan_incr_delete_ws_bytes(long capacity, int d, long chunk);
int mused_dbscan_incr_delete(const double* X, long ld, int d, double* nrm, int* count, int* parent, int* best, long n, long m,
                             double eps, int min_samples, long chunk, int* labels_out, int* info_out, void* ws, long ws_bytes,
                             void* stream);

/* ---- DBSCAN_incr, ANY rows deleted: the rows at the m positions dele[] of the n rows held, csrc/dbscan_incr.hip.  The pin is
 * that of mused_dbscan_incr_delete: afterwards the labels of the n - m rows still held equal sklearn DBSCAN(eps, min_samples,
 * metric="euclidean").fit_predict(those rows, in their order), numbering included (specification: mused_amd/dbscan_incr.py,
 * `delete_rows`).  The same three tile passes with the deleted rows gathered into the staging panel: (deleted rows) x (all
 * rows) for the counts, then the rebuild and the border pass over the survivors.  dele = 0 .. m - 1 leaves the state, labels
 * and info of mused_dbscan_incr_delete(m), bit for bit (parent[] up to the shape of its trees: the roots are the same).
 * NOT enqueue-only: the call reads the list's flag and the two list lengths between its phases.
 * X: the n rows held, fp64 (pitch ld), n <= 2^19; NOT modified.  X_out (pitch ld_out >= d): receives the n - m surviving rows,
 *   packed in their order; it must not overlap the rows held (an error).
 * nrm, count, parent, best: as mused_dbscan_incr_delete; on return entries [0, n - m) describe the survivors in the new
 *   numbering: survivor i has become i - |{ j in dele : j < i }|, parent and best entries are renumbered through the same map.
 * dele: m int32 (DEVICE), strictly ascending, in [0, n); 1 <= m <= n.  A kernel checks the list before anything is written:
 *   a list that is not so sets flag 4 in info_out[0] and every array is left untouched.
 * labels_out: n - m int32 (DEVICE).  info_out (HOST, 6 int32) = {flags (0 or 4), clusters, core rows, rows that lost core
 *   status, |R|, |B|} as mused_dbscan_incr_delete.
 * ws: mused_dbscan_incr_delete_rows_ws_bytes(capacity, d, chunk) bytes for any capacity >= n (56 capacity + 4 ceil(capacity /
 *   128) + 4 ceil(capacity / 1024) + 8 chunk (d rounded up to even) and alignment; -1 as mused_dbscan_incr_delete_ws_bytes).
 *   Outside these limits (m outside [1, n], a short workspace, a bad chunk, d or pitch, an overlap) the call returns an
 *   error and writes nothing. */
long mused_dbscan_incr_delete_rows_ws_bytes(long capacity, int d, long chunk);
int mused_dbscan_incr_delete_rows(const double* X, long ld, int d, double* X_out, long ld_out, double* nrm, int* count, int* parent,
                                  int* best, long n, const int* dele, long m, double eps, int min_samples, long chunk,
                                  int* labels_out, int* info_out, void* ws, long ws_bytes, void* stream);

/* ---- Rows looked up by value, csrc/rows_find.hip: the position of each of q query rows among n held rows, or -1
 * (specification: mused_amd/rows_find.py, which the tests pin it to).  Two rows are equal when all d fp64 values have the same
 * bits: -0.0 is not +0.0, and a NaN row finds a row with the same NaN bits.  A value held at positions h1 < h2 < ... and asked
 * for at query positions q1 < q2 < ...: query q_k gets h_k, and -1 beyond the last held occurrence.  All rows go into one
 * open-addressing table keyed by their bytes (the hash only places a row, the d words identify it), the elements are
 * radix-sorted by the table slot of their value and ranked inside each slot.  Enqueue-only; no pass over values on the host.
 * X: n x d fp64 (pitch ld), Q: q x d fp64 (pitch ldq); n, q >= 0, n + q <= 2^24.
 * idx_out: q int32 (DEVICE).  info_out (DEVICE, 4 int32) = {found, not found, 0, 0}.
 * ws: mused_rows_find_ws_bytes(n, q, d) bytes (40 (n + q) + 1024 ceil((n + q) / 1024) and alignment; -1 outside the limits).
 *   Scratch only.  Outside the limits the call returns an error and writes nothing. */
long mused_rows_find_ws_bytes(long n, long q, int d);
int mused_rows_find(const double* X, long ld, long n, const double* Q, long ldq, long q, int d, int* idx_out, int* info_out,
                    void* ws, long ws_bytes, void* stream);

/* ---- HDBSCAN_batch: the exact Euclidean minimum spanning tree of n fp64 rows, csrc/emst.hip.  For
 * sklearn.cluster.HDBSCAN(min_samples <= 2, metric="euclidean") the mutual-reachability distance is the distance itself, so
 * this tree is the one its Prim loop builds; the sequential rest (Prim's edge order, single-linkage and condensed tree,
 * labels) runs on the host (mused_amd/hdbscan.py, which is also the specification of the rounds).  Boruvka rounds over the
 * fp64 MFMA distance tiles, d2 = max(0, |x_i|^2 + |x_j|^2 - 2 x_i.x_j) recomputed in every round, one evaluation serving
 * both ends of a pair: every component picks its smallest outgoing edge under the total order (d2, min(i, j), max(i, j)),
 * the picks are united by a lock-free union-find.  O(n) workspace: no n x n array, neighbour list or bitmask.  ceil(log2 n)
 * rounds are enqueued; the kernels of the rounds behind the last needed one return at once (a device word).  Enqueue-only.
 * X: n x d fp64 (pitch ld), n <= 2^19 (the tile grid of one launch).
 * edge_a, edge_b (DEVICE, n - 1 int32 each), edge_d2 (DEVICE, n - 1 fp64: the kernel's own d2): the tree's edges in
 *   ARBITRARY order and orientation (the edge SET does not depend on scheduling); may be NULL for n == 1.
 * info_out (DEVICE, 4 int32) = {flags, edges written, rounds run, 0}.  Flags: 1 in some round some outgoing edge of a
 *   component lies within tau(pick) + tau(edge) of its pick, tau(i, j) = 2 (d + 8) 2^-52 (|x_i|^2 + |x_j|^2) + 4 ulp(d2(i, j))
 *   being the bound within which two ways of evaluating d2 can disagree (the second tau is bounded from one end of the
 *   edge: csrc/emst.hip), so another evaluation might pick another tree; 2 a row or a squared distance is not finite;
 *   4 internal error (the two passes of a round disagreed about a distance).  With any flag the edges are NOT to be used:
 *   run the host estimator.
 * ws: mused_emst_ws_bytes(n) bytes (56 n + 4 ceil(n / 128) and alignment; -1 for n outside [1, 2^19]). */
long mused_emst_ws_bytes(long n);
int mused_emst(const double* X, long n, int d, long ld, int* edge_a, int* edge_b, double* edge_d2, int* info_out, void* ws,
               long ws_bytes, void* stream);

/* ---- scoring a run: compute_all_metrics (metrics_evaluation.py:47-92: scikit-learn's NMI, NMI over the rows whose true
 * label is > 0, weighted F1 / precision / recall, accuracy, MAE), csrc/score.hip.  All seven are functions of the
 * true-class x predicted-cluster contingency table (specification: mused_amd/scores.py).  One launch, one workgroup per
 * segment, enqueue-only.
 * truth, pred (DEVICE int32): n_seg consecutive segments of seg_len labels, each scored on its own.
 * out (DEVICE, n_seg x 8 fp64) = {f1, nmi, nmi_e, precision, recall, accuracy, mae, sum |truth - pred|}; accuracy and mae
 *   are one division of exact integers (scikit-learn's bits), the other five carry the rounding of `log` and of the sums.
 * info (DEVICE, n_seg x 8 int32) = {T distinct true values, P distinct predicted values, size of their union, rows with
 *   truth > 0, rows with truth == pred, flags, 0, 0}.  Flags: 4 a label outside [-1, 65534]; 8 T > 4096, P > 4096 or
 *   T * P > cells_cap.  A flagged segment has out = 0: score it on the host.
 * ws: mused_score_ws_bytes(n_seg, cells_cap) bytes (4 n_seg cells_cap); tables above 24,576 cells live there and are cleared
 *   by the kernel, smaller ones stay in LDS.  cells_cap <= 4096^2. */
long mused_score_ws_bytes(long n_seg, long cells_cap);
int mused_score_labels(const int* truth, const int* pred, long n_seg, long seg_len, long cells_cap, double* out, int* info,
                       void* ws, long ws_bytes, void* stream);

/* ---- scoring a partition against the truth whatever the clusters are called, csrc/score_partitions.hip: what ARI, AMI,
 * homogeneity / completeness / V-measure, Fowlkes-Mallows, purity and the matched accuracy are finished from on the host
 * (specification: mused_amd/partition_scores.py, pinned to scikit-learn 1.7.2 and SciPy).  Labels, segments, cells_cap and
 * the flags 4 and 8 as for mused_score_labels.  Up to four launches, enqueue-only: no host read or wait inside the call.
 * want_emi: nonzero asks for the expected mutual information (AMI's correction), about min(T, P) * seg_len terms.
 * out (DEVICE, n_seg x 8 fp64) = {MI, H(truth), H(pred), EMI, 0, 0, 0, 0}, natural logarithms, MI clipped at 0, an entropy
 *   exactly 0 for a side with one value.  Two calls on the same labels give the same bits.
 * ints (DEVICE, n_seg x 8 int64) = {sum n_ij^2, sum a_i^2, sum b_j^2, sum over columns of the column maximum, sum over rows
 *   of the row maximum, number of EMI terms, seg_len, 0}: exact.
 * info (DEVICE, n_seg x 8 int32) = {T, P, flags, 0, 0, 0, 0, 0}.  Flags 4 and 8: out and ints (but seg_len) are 0, score the
 *   segment on the host.  Flag 64: the EMI slot is NaN -- want_emi was 0, seg_len > 2^24 or the segment has more than 2^34
 *   EMI terms (limits that keep one call short); every other output is valid.
 * table_out (DEVICE, may be NULL): n_seg x cells_cap int32; segment s's T x P table, row-major, values in ascending order
 *   on both sides, at s * cells_cap (the cells behind T * P are not written).
 * ws: mused_score_partitions_ws_bytes(n_seg, seg_len, cells_cap) bytes, 8-byte aligned: the log-gamma table (8 (seg_len + 1)
 *   bytes up to seg_len = 2^22; longer segments evaluate lgamma where it is used, the same values), per segment 64 min(seg_len, 4096)
 *   bytes of row partials, a and b (32 KiB) and the table (4 cells_cap), each array rounded up to 256 bytes.
 * MUSED_PARTITION_LGAMMA=direct (read per call): no log-gamma table at any length. */
long mused_score_partitions_ws_bytes(long n_seg, long seg_len, long cells_cap);
int mused_score_partitions(const int* truth, const int* pred, long n_seg, long seg_len, long cells_cap, int want_emi, double* out,
                           long* ints, int* info, int* table_out, void* ws, long ws_bytes, void* stream);

/* ---- scoring clusters WITHOUT ground truth, csrc/silhouette.hip: sklearn.metrics.silhouette_samples(X, labels,
 * metric="euclidean") with the sum of the samples, and davies_bouldin_score / calinski_harabasz_score (specification:
 * mused_amd/silhouette.py, pinned to scikit-learn 1.7).  Any int32 value is a cluster id, -1 included (a cluster like any
 * other).  The rows are ordered by label (stable radix sort, one gathered copy with an even pitch); the silhouette then walks
 * the fp64 MFMA distance tiles row tile by row tile, the columns arriving cluster by cluster, and keeps a running sum, a(i)
 * and the running minimum b(i) per row: O(n + clusters) workspace beside the gathered rows, no n x n and no n x clusters
 * array.  d(i, j) = sqrt(max(0, |x_i|^2 + |x_j|^2 - 2 x_i.x_j)), exactly 0 for i == j; a(i) = own-cluster sum / (size - 1),
 * b(i) = smallest mean over the other clusters, s(i) = (b - a) / max(a, b), 0 for a row alone in its cluster and for 0 / 0.
 * Every sum has one fixed order (no floating-point atomic): two calls on the same inputs give the same bits.  Enqueue-only.
 * X: n x d fp64 (pitch ld), n <= 2^19, d < 2^20.  labels: n int32 (DEVICE).
 * samples_out: n fp64 (DEVICE), the caller's row order.
 * info_out (DEVICE, 16 bytes) = {int32 flags, int32 clusters, fp64 sum of the samples in a fixed order (the score is sum / n)}.
 *   Flags: 2 a row is not finite (or its squared norm overflows); 4 the number of distinct labels is outside [2, n - 1].
 *   With a flag samples_out is NOT written and the sum is NaN: raise what scikit-learn raises.
 * ws: mused_silhouette_ws_bytes(n, d) bytes (32 n + 1024 ceil(n / 1024) + 8 n (d rounded up to even) and alignment; -1 for n
 *   outside [1, 2^19] or d outside [1, 2^20)), plus 32 S n where the column tiles are cut into S = mused_silhouette_slices(n)
 *   > 1 slices (n <= 32,640: S <= 16 runs of whole column tiles, so that about 512 workgroups run; the cut clusters are
 *   closed by a merge kernel in slice order; S depends on n alone).  Scratch only.  Outside these limits, or with a short
 *   workspace, the call returns an error and launches nothing.  MUSED_SIL_SLICES=1 (read per call): one slice. */
long mused_silhouette_ws_bytes(long n, int d);
int mused_silhouette_slices(long n);
int mused_silhouette(const double* X, long n, int d, long ld, const int* labels, double* samples_out, void* info_out, void* ws,
                     long ws_bytes, void* stream);
/* The two cheaper indices from the same sorted order: centroids by a segmented fixed-order reduction, the mean distance of a
 * cluster's rows to its centroid and the sum of their squares (from the differences x - c), the centroid distances, the two
 * dispersions.  O(n d + clusters^2 d) work.
 * out (DEVICE, 2 fp64) = {Davies-Bouldin, Calinski-Harabasz}.  Davies-Bouldin is 0.0 when every mean distance or every
 *   centroid distance is <= 1e-8 (scikit-learn's allclose), a zero centroid distance counts as infinite; Calinski-Harabasz
 *   is 1.0 when the within-cluster dispersion is exactly 0.
 * info_out (DEVICE, 4 int32) = {flags, clusters, 0, 0}, flags as above; with a flag `out` is NOT written.
 * ws: mused_cluster_indices_ws_bytes(n, d) bytes (what mused_silhouette takes + 8 n d + 8 d + 40 n and alignment). */
long mused_cluster_indices_ws_bytes(long n, int d);
int mused_cluster_indices(const double* X, long n, int d, long ld, const int* labels, double* out, int* info_out, void* ws,
                          long ws_bytes, void* stream);

/* ---- DBSCAN's eps from the data, csrc/kdist.hip (specification: mused_amd/kdist.py): the squared distance of every row to
 * its k-th nearest row, THE ROW ITSELF COUNTED (scikit-learn's convention for min_samples and for
 * NearestNeighbors(n_neighbors=k).kneighbors(X)): kd2[i] = the k-th smallest of d2(i, j) over all j,
 * d2 = max(0, |x_i|^2 + |x_j|^2 - 2 x_i.x_j), exactly 0 for j == i.  The full-square schedule of mused_silhouette: a workgroup
 * owns a 128-row tile, walks column tiles of fp64 MFMA products and keeps every row's k smallest values in LDS; only entries
 * below a row's current k-th value leave the accumulators, and none is dropped (rows with more passing entries than staging
 * slots are served in further rounds).  Below 256 row tiles the column tiles are cut into the S <= 16 slices of
 * mused_silhouette_slices(n) and a merge kernel takes the k-th smallest of a row's S lists.  The k-th smallest of a multiset
 * does not depend on the order of arrival: two calls give the same bits; no floating-point atomic.  Two instances, lists of 8
 * (k <= 8) and of 64.  Enqueue-only.
 * X: n x d fp64 (pitch ld >= d), 1 <= n <= 2^19, d < 2^20, 1 <= k <= min(n, 64).
 * kd2_out: n fp64 (DEVICE), SQUARED distances.
 * info_out (DEVICE, 4 int32) = {flags, slices, list length of the instance (8 or 64), 0}.  Flags: 2 a row is not finite (or its
 *   squared norm overflows); kd2_out is NOT written then.
 * ws: mused_kth_distance_ws_bytes(n, k) bytes (16 + 8 n, plus 8 S k n with S > 1 slices, and alignment; -1 outside the limits
 *   above).  Scratch only.  Outside the limits, or with a short workspace, the call returns an error and launches nothing. */
long mused_kth_distance_ws_bytes(long n, int k);
int mused_kth_distance(const double* X, long n, int d, long ld, int k, double* kd2_out, int* info_out, void* ws, long ws_bytes,
                       void* stream);
/* The knee of the sorted k-distance curve and the eps between its knee and the next larger value (mused_amd/kdist.py: knee,
 * eps_from_curve).  v = sqrt(kd2) sorted ascending by bit pattern (eight stable radix passes: low word, then high word);
 * g_i = i / (n - 1) - (v_i - v_0) / (v_{n-1} - v_0); i* = the FIRST maximum of g (a fixed-order reduction, ties to the smaller
 * index); nxt = the first index > i* with v[nxt] > v[i*]; eps = 0.5 (v[i*] + v[nxt]) -- the bits of the NumPy rule.
 * kd2: n fp64 (DEVICE), n <= 2^19, every value finite and >= 0.
 * out (DEVICE, 48 bytes) = {int64 i*, int64 nxt, fp64 v[i*], fp64 v[nxt], fp64 eps, int64 flags}.  Flags: 2 a value of kd2 is
 *   negative or not finite; 4 the curve is flat (v[n-1] == v[0]: always for k = 1 and for n = 1).  With a flag the indices
 *   are -1 and the three numbers NaN.
 * ws: mused_eps_knee_ws_bytes(n) bytes (40 n + 1024 ceil(n / 1024) + 16 and alignment; -1 for n outside [1, 2^19]).  Its
 *   FIRST n doubles hold the sorted curve v after the call, for callers that plot it; the rest is scratch. */
long mused_eps_knee_ws_bytes(long n);
int mused_eps_knee(const double* kd2, long n, void* out, void* ws, long ws_bytes, void* stream);

/* ---- Orthogonal Procrustes, csrc/procrustes.hip (specification: mused_amd/procrustes.py): the orthogonal R (r x r) that
 * minimises |A R - B|_F, the polar factor of M = A^T B -- scipy.linalg.orthogonal_procrustes(A, B), reflections allowed.
 * M by the split-K GEMM (256 rows a split, partials summed in split order), then ONE workgroup: one-sided Jacobi on the columns
 * of M in LDS (round-robin pairs dealt to 16 waves, a pair rotated when (w_p.w_q)^2 > 2^-100 (w_p.w_p)(w_q.w_q), the sweep that
 * rotates nothing is the last, at most 30), sigma_j = |w_j|, U = W / sigma, R0 = U (U^T M / sigma), one Newton-Schulz step
 * R = 1/2 R0 (3 I - R0^T R0).  Fixed summation orders: two calls give the same bits.  Enqueue-only.
 * A, B: m x r fp64 (DEVICE; pitches lda, ldb >= r; A == B allowed), 1 <= m < 2^30, 1 <= r <= 128.  r > 128 returns
 *   MUSED_ERR_UNSUPPORTED (-4) before anything is launched.
 * R_out (DEVICE): r x r fp64, row-major, pitch r.
 * out_f64 (DEVICE, 4 fp64): [0] scale = the sum of the singular values of M, [1] sigma_max, [2] sigma_min, [3] 0.
 * info_out (DEVICE, 4 int32): [0] flags, [1] sweeps run (the last, clean one counted), [2] 0, [3] 0.  Flags: 2 an entry of M is
 *   not finite (an entry of A or B is not, or a product overflowed): R_out is NOT written, out_f64[0 .. 2] are NaN, sweeps 0;
 *   4 sigma_max == 0 or sigma_min <= 2^-14 sigma_max (the data do not determine R: m < r, a zero column, ...); 8 the sweep
 *   cap was hit.  With 4 or 8 R_out holds what the steps gave and is not to be relied on.
 * ws: mused_procrustes_ws_bytes(m, r) bytes (24,576 + 8 r^2 (4 + ceil(m / 256)) and alignment; -1 outside the limits above).
 *   Scratch only. */
long mused_procrustes_ws_bytes(long m, int r);
int mused_procrustes(const double* A, long lda, const double* B, long ldb, long m, int r, double* R_out, double* out_f64,
                     int* info_out, void* ws, long ws_bytes, void* stream);
/* out = E R for the n rows of a window (R: r x r row-major, pitch r, staged in LDS), and, with Bref, the three sums over
 * the first m rows: sums_out[0] = |E[:m] R - Bref|_F^2, [1] = |Bref|_F^2, [2] = |E[:m] - Bref|_F^2 -- per-workgroup partials
 * added in index order by a second launch, no floating-point atomic: two calls give the same bits.  Enqueue-only.
 * E: n x r fp64 (pitch lde), out: n x r fp64 (pitch ldo), MUST NOT overlap E (checked: MUSED_ERR_ARG); 1 <= n < 2^30,
 * r <= 128 (beyond: MUSED_ERR_UNSUPPORTED).  Bref: m x r fp64 (pitch ldb), 1 <= m <= n, or NULL (no sums; sums_out and m ignored).
 * sums_out: 3 fp64 (DEVICE).  ws: at least 24,576 bytes of scratch (a workspace of mused_procrustes serves). */
int mused_procrustes_apply(const double* E, long lde, long n, int r, const double* R, double* out, long ldo, const double* Bref,
                           long ldb, long m, double* sums_out, void* ws, void* stream);
/* The SVD kernel of mused_procrustes alone, for direct tests: W_out (r x r, row-major, pitch r) = M V, the columns of M after
 * the Jacobi sweeps (mutually orthogonal to the rotation threshold), sigma_out[j] = |column j of W_out| (r fp64, NOT sorted),
 * info_out as above.  M: r x r fp64 row-major (DEVICE, pitch ldm >= r), r <= 128.  With flag 2 only info_out is written. */
int mused_svd_jacobi_small(const double* M, long ldm, int r, double* W_out, double* sigma_out, int* info_out, void* stream);

/* ---- a5-a7: SeqBasedSWFD (swfd submodule; call sites main.py:62,65-67,70) ---------------------- */

/* SeqBasedSWFD(N=, R=, d=, sketch_dim=) */
int mused_swfd_create(long N, double R, int d, int sketch_dim, int sweeps, void** handle);
/* `lanes` independent sketch sets advanced in lockstep by the same launches (windows of `lanes`
 * contiguous blocks of the stream): sketches, queries and outputs get a leading lane dimension */
int mused_swfd_create_lanes(long N, double R, int d, int sketch_dim, int sweeps, int lanes, void** handle);
int mused_swfd_lanes(void* handle);
/* n_rows rows for every lane; lane b reads rows + b * lane_stride (elements) */
int mused_swfd_append_lanes(void* handle, const void* rows, int dtype, long n_rows, long ld, long lane_stride,
                            void* stream);
int mused_swfd_destroy(void* handle);
int mused_swfd_levels(void* handle);
/* live timing of the rotation eigensolver: HIP events around every Jacobi sweep graph; read is BLOCKING and
 * returns summed ms, number of osj_round_kernel launches covered, bytes one launch streams (HOST outputs) */
int mused_swfd_profile(void* handle, int on);
int mused_swfd_profile_read(void* handle, double* total_ms, long* launches, double* bytes_per_launch);
/* the same for sketches whose rotations run a direct eigensolver (csrc/trd.hip: orders 2 l <= 256; csrc/trdx.hip: 320 .. 1024): ms of the solver-chain launches (trd_a .. trd_d), their
 * number, matrices they solved; *direct = 0 -> the rotations run the Jacobi, use mused_swfd_profile_read (HOST outputs) */
int mused_swfd_profile_read_direct(void* handle, double* total_ms, long* launches, double* matrices_solved, int* direct,
                                   double* tridiag_ms /* may be NULL: the share of total_ms spent in trd_a_kernel */);
/* .fit(row) for n_rows rows at once (any batching gives the same sketch) */
int mused_swfd_append(void* handle, const void* rows, int dtype, long n_rows, long ld, void* stream);
/* .get(): out_sketch (lanes x sketch_dim x d), out_sigma (lanes x sketch_dim, may be NULL),
 * out_info (lanes x 2 = {level, delta}, may be NULL) */
int mused_swfd_query(void* handle, double* out_sketch, double* out_sigma, double* out_info, void* stream);
int mused_swfd_counters(void* handle, long* rows_seen, int* pending); /* HOST outputs */
/* BLOCKING (synchronises `stream`): *status_out (HOST) != 0 -> an eigensolve of this sketch gave up (bit 0: timeout of the
 * persistent work-queue solver); everything it has returned since is invalid.  Sticky. */
int mused_swfd_status(void* handle, int* status_out, void* stream);
/* state exchange between ranks (one half = the L sketches of kind 0 MAIN / 1 AUX; single-lane handles) */
long mused_swfd_half_bytes(void* handle);
/* Packs one half into dst (device, mused_swfd_half_bytes bytes).  THE EXCHANGE FORMAT, with L = mused_swfd_levels,
 * l = sketch_dim, every part level-major and without padding:
 *   [ buffers     L x 2l x d  f64 | snapshot rings  L x 2l x d  f64 | timestamps  L x 2l  i64 | meta  L x 4  i32 | dropped  L  i64 ]
 * buffer of a level: rows 0 .. nk - 1 the kept rows, then the rows appended since the last rotation, then zeros;
 * meta = {nk, ring head, ring count, dumps the next level did not make}: the live snapshots are the ring slots
 * (head + q) mod 2l, q < count, oldest first, timestamps (row numbers, from 1) at the same slots -- slots outside that
 * range hold stale data; dropped = the largest timestamp of a snapshot lost to the ring capacity (0: none).
 * A MAIN level below the top that has lost a snapshot of the current epoch is frozen until the epoch ends (it cannot be
 * selected before AUX replaces it): its exported state is the one of its last rotation. */
int mused_swfd_export_half(void* handle, int kind, void* dst, void* stream);
/* the inverse: overwrites one half with a blob of the same N, R, d, sketch_dim (row counter and pending rows untouched) */
int mused_swfd_import_half(void* handle, int kind, const void* src, void* stream);
int mused_swfd_begin_epoch(void* handle, long rows_seen, const void* main_half, void* stream);
/* BLOCKING unit primitive: one FD rotation of a (2 l x d) buffer in place */
int mused_fd_rotate(double* buf, int ell, int d, double* sigma_out, int sweeps, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MUSED_HIP_H */
