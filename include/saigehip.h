/*
 * saigehip.h -- C ABI of libsaigehip.so, the MI355X (gfx950) implementation of
 * the SAIGEgds single-variant association scan.
 *
 * Drop-in boundary.  In the reference the R driver seqAssocGLMM_SPA()
 * (R/assoc_single.r:92-334) reaches native code through three .Call entry
 * points, the last two ONCE PER VARIANT from SeqArray::seqApply
 * (R/assoc_single.r:207,218 via .cfunction, R/saige_main.r:22-30):
 *
 *   SEXP saige_score_test_init (SEXP model)    src/saige_main.cpp:103-150
 *   SEXP saige_score_test_bin  (SEXP dosage)   src/saige_main.cpp:437-462
 *   SEXP saige_score_test_quant(SEXP dosage)   src/saige_main.cpp:413-434
 *
 * A per-variant callback cannot feed a GPU, so this ABI keeps the meaning of
 * those three calls and changes the granularity to BLOCKS of variants:
 *
 *   sgx_init        <- saige_score_test_init : model arrays by pointer+length,
 *                      copied to HBM (the reference borrows R-owned memory)
 *   sgx_scan_2bit   <- saige_score_test_bin/quant over a block; genotypes are
 *                      2-bit codes, what seqApply(.useraw=NA) yields as RAW
 *                      0/1/2/0xFF, packed 4 samples per byte
 *   sgx_scan_u8     <- the RAWSXP branch of get_ds  (saige_main.cpp:179-182)
 *   sgx_scan_f64    <- the REALSXP branch of get_ds (saige_main.cpp:173-174)
 *
 * Results: one row of 8 doubles per variant,
 *   [AF.alt, mac, num, beta, SE, pval, p.norm, converged]
 * exactly the NumericVector(8) of saige_score_test_bin (saige_main.cpp:453-458);
 * for quantitative traits the reference returns 6 values (:427-430) and columns
 * 6,7 are NaN here.  A variant rejected by the MAF/MAC/missing filter
 * (saige_main.cpp:288-292, :197-201; reference returns R_NilValue) gets
 * valid[j]=0 and a NaN row.
 *
 * No R, torch or HIP types appear in the signatures.  All functions return 0 on
 * success or a negative SGX_E* code; sgx_last_error() gives the message (the R
 * glue turns it into stop(), as BEGIN_RCPP/END_RCPP does in the reference).
 */
#ifndef SAIGEHIP_H
#define SAIGEHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SGX_OK          0
#define SGX_EINVAL     -1   /* bad argument (length, alignment, NULL)          */
#define SGX_EHIP       -2   /* HIP runtime error                               */
#define SGX_ENOMEM     -3   /* allocation failed                               */
#define SGX_ENODEV     -4   /* no usable gfx950 device                         */
#define SGX_ENOSPACE   -5   /* output buffer too small: the needed size is returned */
#define SGX_ERANK      -6   /* sgx_grm_pca: the block of vectors lost rank     */

#define SGX_MAX_COEFF  16   /* K = nrow(XV) supported by the compiled kernels  */
#define SGX_TRAIT_BINARY 0
#define SGX_TRAIT_QUANT  1

/* 2-bit genotype code (alt-allele dosage, SeqArray "$dosage_alt"); sample i of a
 * variant row lives in bits 2*(i%4)..2*(i%4)+1 of byte i/4. */
#define SGX_GENO_MISSING 3

typedef struct sgx_handle sgx_handle;

/* The list .init_nullmod builds (R/assoc_single.r:28-66) as read by
 * saige_score_test_init (src/saige_main.cpp:106-130).  K x N matrices are
 * column-major, i.e. the K values of sample i are contiguous at [K*i].
 *
 * t_XXVX_inv and XV are part of the reference's list and are accepted here so
 * that the caller passes the list as it is, but the scan does not read them:
 * both reference branches (saige_main.cpp:237-262 sparse, :263-292 dense) are
 * computed from t_X, t_XVX_inv_XV, XVX and S_a.  They may be
 * NULL.  With SAIGEHIP_CHECK_MODEL=1 in the environment sgx_init holds them
 * against t_X / t_XVX_inv_XV (XV = V t_X, t_XVX_inv_XV = V t_XXVX_inv with one
 * weight V_i per sample, 1e-8) and returns SGX_EINVAL naming the first entry
 * that disagrees -- for callers who assemble the arrays themselves. */
typedef struct sgx_model {
	int32_t n_samp;              /* N  = length(y)                  :117 */
	int32_t n_coeff;             /* K  = nrow(XV)                   :118 */
	int32_t trait;               /* SGX_TRAIT_*                          */
	int32_t reserved;
	double tau[2];               /* variance components             :119 */
	double var_ratio;            /* var.ratio                       :130 */
	double maf;                  /* thresholds; NaN -> -1/-1/1/0.05 :108-115 */
	double mac;
	double missing;
	double spa_pval;
	const double *y;             /* N                               :120 */
	const double *mu;            /* N                               :121 */
	const double *y_mu;          /* N   y - mu                      :122 */
	const double *mu2;           /* N   mu*(1-mu)                   :123 */
	const double *t_XXVX_inv;    /* K x N   NOT READ by the scan    :124 */
	const double *XV;            /* K x N   NOT READ by the scan    :125 */
	const double *t_XVX_inv_XV;  /* K x N                           :126 */
	const double *XVX;           /* K x K                           :127 */
	const double *t_X;           /* K x N                           :128 */
	const double *S_a;           /* K                               :129 */
} sgx_model;

/* Counters and device timings of the most recent scan call on a handle. */
typedef struct sgx_stats {
	uint64_t n_variants;   /* variants in the call                            */
	uint64_t n_valid;      /* passed the filter                               */
	uint64_t n_spa;        /* pval_noadj <= spa.pval, handed to the SPA stage */
	uint64_t n_spa_dense;  /* of those, needed the exact dense g_pos/g_neg pass */
	uint64_t n_spa_slow;   /* of those, through the exact exp/log kernel (not the series) */
	float ms_score;        /* HIP-event time of the score kernel(s), ms       */
	float ms_spa;          /* HIP-event time of the SPA kernel(s), ms         */
	float ms_total;        /* first launch .. last launch complete, ms        */
	uint32_t score_launches;
	uint32_t spa_launches;
	float ms_kernel;       /* HIP-event time of the genotype-streaming kernel alone (score3_kernel), ms;
	                          0 where the scan took the FP64 kernels                                      */
	float ms_lists;        /* row-major calls on the two-plane form: HIP-event time of the pass that finds the
	                          missing genotypes (in front of the score stage; part of ms_total, not of
	                          ms_score); 0 for the three-plane form and for sgx_scan_block, whose lists were
	                          made when the block was loaded                                             */
	uint32_t three_plane;  /* 1: the call took the three-plane form of the contraction kernel (the sums over the
	                          missing samples from a third MFMA plane: no lists, no sparse pass; chosen for
	                          few score columns or many missing genotypes); totals: number of such calls.
	                          0 for a call of the FP64 kernels (score_v1, or a model outside the fixed-point form) */
	uint32_t n_unlisted;   /* variants of a two-plane call whose missing genotypes are not listed, scored by the FP64
	                          kernel instead (same results): a row-major call lists at most 256 missing genotypes of a
	                          (variant, sample range) segment, a resident block what the pool of its lists has room
	                          for; 0 in the three-plane form and for the FP64 kernels                               */
	uint32_t n_guarded;    /* variants whose a-posteriori bound on the fixed-point columns' quantisation (its
	                          effect on the z-score) exceeded the guard: scored by the FP64 kernel  */
} sgx_stats;

/* Library / device ------------------------------------------------------- */
const char *sgx_version(void);
const char *sgx_last_error(void);
int sgx_device_count(void);
/* verifies the v_mfma_i32_16x16x64_i8 lane maps the score kernel relies on and
 * the accuracy of the device exp/log used by the SPA stage */
int sgx_selftest(int device);

/* Model lifetime (one handle per GPU; handles are independent, no globals). */
int  sgx_init(const sgx_model *model, int device, sgx_handle **out);
void sgx_free(sgx_handle *h);
int  sgx_set_thresholds(sgx_handle *h, double maf, double mac, double missing,
	double spa_pval);

/* Fixed-point layout sgx_init chose for the exact-integer score stage: limbs[c] = bytes per entry of
 * score column c in the order c' (K columns), e (K), s, w; 0 for a column that is derived instead
 * of carried.  Columns of heavy-tailed covariates get more limbs than ordinary ones; n_groups = 0
 * means the model's dynamic range exceeds what the fixed-point form holds and the scan uses the
 * FP64 kernels. */
int sgx_score_layout(sgx_handle *h, int32_t *limbs, int32_t n_limbs, int32_t *n_groups);

/* Scan a block of variants held in HOST memory.  packed: n_variants rows of
 * bytes_per_variant bytes (>= ceil(N/4)).  out8: n_variants*8 doubles.
 * valid: n_variants bytes.  Synchronous (chunks cross PCIe while the previous chunk is scanned). */
int sgx_scan_2bit(sgx_handle *h, const uint8_t *packed, size_t bytes_per_variant,
	size_t n_variants, double *out8, uint8_t *valid);

/* Page-locked host memory for block buffers handed to the host-buffer scans: from it the chunks cross
 * PCIe at the full link rate and asynchronously (pageable memory works too, staged by the runtime). */
void *sgx_host_alloc(size_t bytes);
void  sgx_host_free(void *p);

/* Device and pinned bytes held right now by everything the library owns in this process: handles, blocks,
 * operators and the scratch of calls in progress, over all devices.  It rises when an object is made or one of
 * its workspaces grows and is back where it was once the object is freed; memory from sgx_host_alloc is the
 * caller's and is not counted.  A test of ownership, not an accounting of the device. */
size_t sgx_live_bytes(void);

/* Same, all buffers already resident in this GPU's HBM (device pointers): the headline path.
 * packed must be 16-byte aligned and bytes_per_variant a multiple of 64 with
 * bytes_per_variant >= sgx_row_stride(N) = 128*ceil(N/512) (rows that start on 128-byte lines are read
 * as whole lines; a stride that is a multiple of 64 only still works, slower).  The rows are read WHERE
 * THEY ARE, twice: one pass lists the positions of the missing genotypes (the sparse form of
 * f64_af_ac_impute's walk, src/vectorization.cpp:186-205), then the contraction kernel streams them;
 * nothing is copied or rearranged.  Asynchronous on one of the handle's streams: the rows, out8_dev and
 * valid_dev must stay untouched until sgx_sync(), which is also what makes results and stats readable. */
int sgx_scan_2bit_dev(sgx_handle *h, const uint8_t *packed_dev,
	size_t bytes_per_variant, size_t n_variants, double *out8_dev,
	uint8_t *valid_dev);

/* Genotype blocks: rows resident on the device for any number of scans ------------------------------
 * The reference streams one variant at a time out of the GDS file into its C++ code
 * (R/assoc_single.r:202-209, seqApply) and finds, per variant and per phenotype, the missing genotypes
 * (f64_af_ac_impute) and the carriers (f64_nonzero_index, src/vectorization.cpp:209-215).  A BLOCK keeps
 * up to max_variants rows in HBM together with what does not depend on the model: the rows themselves
 * (row-major, as they came), the positions of their missing genotypes, and the carrier lists (sample and
 * code, ascending) of every variant with at most 8 192 carriers in the orientation the scan will use
 * (non-zero codes, or the codes other than 2 where the alt allele is the major one).  One loaded block
 * can be scanned with any number of models (phenotypes): each scan then streams the rows once.
 *   sgx_block_create    device storage for up to max_variants rows of n_samp samples
 *   sgx_block_bytes     what that takes (about 1.2 x the packed rows at large N)
 *   sgx_block_load_dev  rows already in this GPU's memory (bytes_per_variant a multiple of 16,
 *                       >= sgx_row_stride(n_samp), 16-byte aligned); asynchronous on the handle's stream;
 *                       a load waits for the scans that still read the block
 *   sgx_block_load      rows in host memory (>= ceil(n_samp / 4) bytes each), through the pinned pipeline
 *   sgx_scan_block      the scan; asynchronous like sgx_scan_2bit_dev (same lanes, stats, sgx_sync)
 *   sgx_block_create_ex test hook: carrier lists with room for clist_avg entries per variant on average
 * A block must not be freed, and its result buffers not read, before sgx_sync() on every handle that
 * scanned it.  Variants whose missing genotypes find the block's pool full (a list entry per missing
 * genotype, room for 0.8 % of the block at large N) are scanned by the FP64 kernels instead: same
 * results, slower.  Rare variants beyond a full carrier list (1 536 entries per variant of the block
 * on average) have their rows scanned by the SPA kernels, as sgx_scan_2bit_dev's rows are: same results. */
typedef struct sgx_block sgx_block;
size_t sgx_block_bytes(int32_t n_samp, size_t max_variants);
int  sgx_block_create(int32_t n_samp, size_t max_variants, int device, sgx_block **out);
int  sgx_block_create_ex(int32_t n_samp, size_t max_variants, int device, long long clist_avg, sgx_block **out);
void sgx_block_free(sgx_block *b);
int  sgx_block_load_dev(sgx_handle *h, sgx_block *b, const uint8_t *packed_dev,
	size_t bytes_per_variant, size_t n_variants);
int  sgx_block_load(sgx_handle *h, sgx_block *b, const uint8_t *packed,
	size_t bytes_per_variant, size_t n_variants);
size_t sgx_block_variants(const sgx_block *b);
int  sgx_scan_block(sgx_handle *h, const sgx_block *b, double *out8_dev, uint8_t *valid_dev);

/* Dosage inputs in HOST memory, one row of N values per variant, the three branches of get_ds
 * (src/saige_main.cpp:171-183):
 *   u8 : 0..254, 0xFF = missing (RAWSXP :179-182);  i32: NA_INTEGER (INT_MIN) = missing (INTSXP
 *   :175-178);  f64: NaN/Inf = missing (REALSXP :173-174).
 * u8 / i32 blocks that hold hard calls only (0, 1, 2, missing) are packed to 2-bit rows on the device
 * and take the same kernels as sgx_scan_2bit; anything else takes the dosage kernels.
 * All host-buffer scans are pipelined: the next chunk of the block crosses PCIe while the current
 * one is computed ("pipe_mb" option = chunk size). */
int sgx_scan_u8(sgx_handle *h, const uint8_t *dosage, size_t n_variants,
	double *out8, uint8_t *valid);
int sgx_scan_i32(sgx_handle *h, const int32_t *dosage, size_t n_variants,
	double *out8, uint8_t *valid);
int sgx_scan_f64(sgx_handle *h, const double *dosage, size_t n_variants,
	double *out8, uint8_t *valid);

/* Packed-real dosage rows in HOST memory, as a SeqArray file stores annotation/format/DS/data: one row of
 * n_file_samp values per variant, the FILE's samples in the file's order,
 *   SGX_PR_U8 / _I8   1 byte a value,  0xFF   / -128   = missing (dPackedReal8U / dPackedReal8)
 *   SGX_PR_U16 / _I16 2 bytes a value, 0xFFFF / -32768 = missing (dPackedReal16U / dPackedReal16)
 *   SGX_PR_F32        float, NaN / Inf = missing; scale and offset are not applied (dFloat32)
 * with the node's scale and offset: dosage = raw * scale + offset, the product rounded and then the sum (what
 * gdsfmt's reader and saigegds_amd/gds.py compute).  The rows cross PCIe as they are stored -- 1/8, 1/4 or 1/2
 * of the bytes of the float64 rows seqApply hands get_ds (REALSXP, src/saige_main.cpp:173-174) -- and are decoded
 * and sample-selected on the device.  sel: NULL (then n_file_samp must equal the model's n_samp) or n_samp
 * indices into the file's samples in the MODEL's order, each checked against [0, n_file_samp).  Chunks are
 * those of sgx_scan_f64 (rows of 8 n_samp bytes per "pipe_mb"), so out8 / valid equal sgx_scan_f64 on the
 * host-decoded, sample-selected rows bit for bit.  A bad argument (unknown cls, NULL buffer, n_file_samp <
 * n_samp, no sel with n_file_samp != n_samp, an index out of range) returns SGX_EINVAL and launches nothing. */
#define SGX_PR_U8 0   /* dPackedReal8U  */
#define SGX_PR_I8 1   /* dPackedReal8   */
#define SGX_PR_U16 2  /* dPackedReal16U */
#define SGX_PR_I16 3  /* dPackedReal16  */
#define SGX_PR_F32 4  /* dFloat32       */
int sgx_scan_packed(sgx_handle *h, const void *raw, int cls, size_t n_file_samp, double scale, double offset,
	const int32_t *sel, size_t n_variants, double *out8, uint8_t *valid);

/* Hard calls in HOST memory as a SeqArray file stores genotype/data (dBit2 [row][sample][ploidy]): per sample one
 * nibble, allele a0 in bits 0-1 and a1 in bits 2-3, n_file_samp samples a row -- the FILE's samples in the file's
 * order -- and the rows back to back in one bit stream, so with an odd n_file_samp every other row starts in the
 * middle of a byte.  alleles: the bytes that hold the variants' rows; the first row starts at bit `bit0` (0 or 4) of
 * the first byte.  n_rows: NULL (one row per variant) or the rows of each variant (genotype/@data; 1 to 16: a site of
 * more than three alleles takes several rows, the base-4 digits of the allele index, least significant first; an
 * allele is missing when all its digits are 3 and non-reference when any digit is non-zero and it is not missing).
 * sel: NULL (then n_file_samp must equal the model's n_samp) or n_samp indices into the file's samples in the
 * MODEL's order, each checked against [0, n_file_samp).  The rows cross PCIe as stored, 4 bits a sample, and are
 * folded into the 2-bit rows of sgx_scan_2bit on the device, by the rule of sgx_decode_dbit2: code 3 if an allele is
 * missing, else the number of non-reference alleles.
 *   sgx_scan_dbit2        chunks of as many variants as sgx_scan_2bit's (2-bit rows of the device stride per
 *                         "pipe_mb"); the raw chunk i + 1 crosses the link while chunk i is decoded and scanned.
 *                         out8 / valid equal sgx_scan_2bit on sgx_decode_dbit2's rows bit for bit.
 *   sgx_block_load_dbit2  sgx_block_load of the same rows: the loaded block gives the same sgx_scan_block tables
 *                         bit for bit, with the same readiness guarantee.
 * A bad argument (NULL buffer, bit0 other than 0 and 4, n_file_samp < n_samp, no sel with n_file_samp != n_samp, an
 * index out of range, n_rows[j] < 1 or > 16) returns SGX_EINVAL and launches nothing; the handle stays usable. */
int sgx_scan_dbit2(sgx_handle *h, const uint8_t *alleles, size_t bit0, size_t n_file_samp,
	const int32_t *n_rows, const int32_t *sel, size_t n_variants, double *out8, uint8_t *valid);
int sgx_block_load_dbit2(sgx_handle *h, sgx_block *b, const uint8_t *alleles, size_t bit0, size_t n_file_samp,
	const int32_t *n_rows, const int32_t *sel, size_t n_variants);

/* Aggregate tests: n_rows burden rows from 2-bit genotypes in HOST memory, then the
 * single-variant test on every row (replaces ds_mat_burden + single_test_bin/quant inside
 * saige_burden_test_*, saige_acatv_test_bin and saige_acato_test_bin, src/saige_main.cpp:526-976).
 * Row r = sum over its entries e in [row_ptr[r], row_ptr[r+1]) of lut[4e + code], code = the 2-bit
 * genotype of variant var_idx[e] (row of `packed`); the caller folds weight, mean imputation and
 * the flip to the minor allele into lut (see saigegds_amd/aggregate.py).  out8 / valid as above,
 * one row per burden row.  Synchronous. */
int sgx_burden_2bit(sgx_handle *h, const uint8_t *packed, size_t bytes_per_variant,
	size_t n_variants, size_t n_rows, const int64_t *row_ptr, const int32_t *var_idx,
	const double *lut, double *out8, uint8_t *valid);

/* SKAT set test: per unit the score statistics of its variants and their covariance, from 2-bit genotypes in HOST
 * memory (nothing of this is in the reference, which has no variance-component test).  Unit u has the
 * entries e in [unit_ptr[u], unit_ptr[u+1]) = rows var_idx[e] of `packed`, each with a 4-entry dosage table
 * lut[4e + code] that holds mean imputation and the flip to the minor allele as for sgx_burden_2bit (no weight).  With
 * G_e the dosage vector that table gives and adj_e = G_e - X (X'VX)^-1 X'V G_e as in the single-variant test:
 *   score[e]                 S_e = sum_i (y - mu)_i adj_ei                    (quantitative traits: divided by tau[0])
 *   cov, unit u: m_u x m_u doubles, row-major, at the sum of m_v^2 over the units v < u, exactly symmetric:
 *                            Phi_ef = var_ratio * sum_i mu2_i adj_ei adj_fi   (quantitative traits: mu2 = 1)
 * so that S_e^2 / Phi_ee is the chi-square behind the p.norm column of the scan of that variant.  The sums are made in
 * FP64 on the matrix cores in a fixed order: no atomics, the same bits from call to call, and what a unit gets does
 * not depend on the other units of the call or on their order.  An entry whose table holds a non-finite value gets
 * non-finite results and leaves the other entries of its unit alone.  The rows cross PCIe once per call in the chunks
 * of the host-buffer scans.  A unit of 0 entries is legal and writes nothing; a unit of more than
 * SGX_SKAT_MAX_VARIANTS entries, a variant index outside [0, n_variants) or a NULL buffer returns SGX_EINVAL and
 * launches nothing; the handle stays usable.  Synchronous. */
#define SGX_SKAT_MAX_VARIANTS 4096
int sgx_skat_2bit(sgx_handle *h, const uint8_t *packed, size_t bytes_per_variant, size_t n_variants,
	size_t n_units, const int64_t *unit_ptr, const int32_t *var_idx, const double *lut,
	double *score, double *cov);

/* Conditional scan: the score statistic of every scanned variant, its variance and its covariances with a set C of
 * conditioning (lead) variants -- what the test of variant j given C needs (saigegds_amd/cond.py; nothing of this is in
 * the reference, DESIGN.md 8b "Conditional analysis").  Tables as for sgx_skat_2bit: lut[4j + code] holds mean imputation
 * and the flip to the minor allele.  With S and Phi as sgx_skat_2bit defines them:
 *   sgx_cond_set       installs the set: n_cond (1 .. SGX_COND_MAX) 2-bit rows in HOST memory with their tables.
 *                      score_c[n_cond] = S_C and cov_cc[n_cond][n_cond] = Phi_CC, exactly symmetric, are made by the
 *                      functions sgx_skat_2bit is made of and equal sgx_skat_2bit on the set as one unit bit for bit.
 *                      The handle keeps the set's sums and the dense matrix the kernel multiplies by
 *                      (n_samp x 16 ceil((2K + 1 + n_cond) / 16) doubles on the device).  A later call replaces the set
 *                      once everything queued on the handle has finished; n_cond = 0 clears it.  Synchronous.
 *   sgx_cond_2bit      rows in HOST memory, uploaded in the chunks of the host-buffer scans:
 *                        score[j] = S_j,  var[j] = Phi_jj,  cov[j * n_cond + c] = Phi_jc,
 *                      so that S_j^2 / Phi_jj is the chi-square behind the p.norm column of the scan of that row.
 *                      Synchronous; a thin wrapper around the next entry: same kernel, same bits.
 *   sgx_cond_2bit_dev  the same from rows in DEVICE memory (stride and alignment as for sgx_scan_2bit_dev); tables and
 *                      results are device pointers.  Asynchronous on the stream of the handle's most recently issued
 *                      call, so it is ordered behind a scan of the same rows; results are readable after sgx_sync().
 * The sums are made in FP64 on the matrix cores (Phi_jj's quadratic term on the vector ALU) in a fixed order: no atomics,
 * sample slabs cut by n_samp alone, so a row's results do not depend on the number of rows, on the row's position, on the
 * other rows of the call or on how the call is cut into chunks.  A row whose table holds a non-finite value gets
 * non-finite results and leaves the other rows alone.  n_variants = 0 succeeds and does nothing.  A NULL buffer,
 * n_cond > SGX_COND_MAX, bytes_per_variant < ceil(n_samp / 4), a bad device stride or alignment, or sgx_cond_2bit* with no
 * set installed returns SGX_EINVAL and launches nothing; the handle stays usable. */
#define SGX_COND_MAX 16
int sgx_cond_set(sgx_handle *h, const uint8_t *packed_c, size_t bytes_per_variant, size_t n_cond,
	const double *lut_c, double *score_c, double *cov_cc);
int sgx_cond_2bit(sgx_handle *h, const uint8_t *packed, size_t bytes_per_variant, size_t n_variants,
	const double *lut, double *score, double *var, double *cov);
int sgx_cond_2bit_dev(sgx_handle *h, const uint8_t *packed_dev, size_t bytes_per_variant, size_t n_variants,
	const double *lut_dev, double *score_dev, double *var_dev, double *cov_dev);

/* Firth bias-reduced effect size of a binary-trait row (saigegds_amd/firth.py; nothing of this is in the reference,
 * DESIGN.md 8j).  Tables as for sgx_skat_2bit / sgx_cond_2bit: g_i = lut[4j + code_i].  With the model's fitted mean mu as
 * offset, logit p_i = logit mu_i + beta g_i, w_i = p_i (1 - p_i) and, over the samples with g_i != 0,
 *   I = sum w g^2,  A = sum w (1 - 2p) g^3,  B = sum w (1 - 6w) g^4,  U* = sum g (y - p) + A / 2I
 * (U*: the score of loglik + 1/2 log I), the result is the root of U*:
 *   out4[4j .. 4j + 3] = {beta, SE = 1 / sqrt(I(beta)), iterations, converged (1 / 0)}
 * for the table's orientation (a driver negates beta of a flipped row).  The root is found by Newton's iteration from 0
 * with Fisher scoring's step where dU* / dbeta >= 0, steps capped at +-5 and bisected into the sign bracket once both its
 * ends are known, to |step| <= 1e-12 max(1, |beta|) in at most maxit iterations.  A row with no non-zero dosage
 * (I = 0) or a non-finite table value gets {NaN, NaN, ., 0}; a row that runs out of iterations {beta of the last
 * iterate, NaN, maxit, 0}; neither disturbs another row.
 *   sgx_firth_2bit      rows in HOST memory, uploaded in the chunks of the host-buffer scans.  Synchronous; a thin
 *                       wrapper around the next entry: same kernel, same bits.
 *   sgx_firth_2bit_dev  rows in DEVICE memory (stride and alignment as for sgx_scan_2bit_dev); table and results are
 *                       device pointers.  Asynchronous on the handle's stream; results are readable after sgx_sync().
 * One workgroup per row, FP64 sums in a fixed order, no atomics: a row's results depend on the row, its table and the
 * model only -- not on its position, the other rows, the grid or the chunks.  Lists that do not fit LDS go to a scratch
 * buffer the handle allocates on first use and frees with itself.  n_variants = 0 succeeds and does nothing.  A
 * quantitative-trait handle, a NULL buffer, bytes_per_variant < ceil(n_samp / 4), a bad device stride or alignment, or
 * maxit < 1 returns SGX_EINVAL and launches nothing; the handle stays usable. */
int sgx_firth_2bit(sgx_handle *h, const uint8_t *packed, size_t bytes_per_variant, size_t n_variants,
	const double *lut, int maxit, double *out4);
int sgx_firth_2bit_dev(sgx_handle *h, const uint8_t *packed_dev, size_t bytes_per_variant, size_t n_variants,
	const double *lut_dev, int maxit, double *out4_dev);

/* Exact p-value of a binary-trait row with few minor alleles (saigegds_amd/exact.py; SAIGE proper's "efficient
 * resampling"; nothing of this is in the reference).  Table as above, t = lut[4j .. 4j + 3], g_i = t[code_i];
 * it is valid when t[1] == 1, (t[0], t[2]) is (0, 2) or (2, 0) and t[3] is finite.  Carriers: the samples with code 0..2
 * and g_i in {1, 2}, in ascending sample order; MAC = sum g_i over them.  Samples with code 3 (imputed to t[3]) are not
 * resampled: delta = t[3] * sum_{code 3} (y_i - mu_i).  The scan's score is T = A - m' with A = sum_carriers g_i y_i, an
 * integer in 0..MAC, and m' = sum_carriers g_i mu_i - delta.  Under the null the carriers' y_i are independent
 * Bernoulli(mu_i): the pmf f of A starts as [1, 0, ...] and takes a carrier by f[a] <- (1 - mu_i) f[a] + mu_i f[a - g_i].
 * With d_a = |a - m'| and d_obs = |A_obs - m'| in double, summed over ascending a,
 *   p.full = sum_{d_a >= d_obs} f[a],     p.mid = sum_{d_a > d_obs} f[a] + 0.5 sum_{d_a == d_obs} f[a],
 *   out4[4j .. 4j + 3] = {p.mid, p.full, MAC, done};
 * done = 0 with NaN p-values for MAC == 0, MAC > max_mac or an invalid table (then out4[4j + 2] = 0 too); none of these
 * disturbs another row.  The samples are taken as independent: neither the variance ratio nor the GRM enters.
 *   sgx_exact_2bit      rows in HOST memory, uploaded in the chunks of sgx_firth_2bit.  Synchronous; a thin wrapper
 *                       around the next entry: same kernel, same bits.
 *   sgx_exact_2bit_dev  rows in DEVICE memory (stride and alignment as for sgx_scan_2bit_dev); table and results are
 *                       device pointers.  Asynchronous on the handle's stream; results are readable after sgx_sync().
 * One wave per row, one pass over the row, FP64 sums in a fixed order, no atomics, no scratch: a row's results depend on
 * the row, its table and the model only -- not on its position, the other rows, the grid or the chunks.  n_variants = 0
 * succeeds and does nothing.  max_mac outside 1..SGX_EXACT_MAX_MAC, a quantitative-trait handle, a NULL buffer,
 * bytes_per_variant < ceil(n_samp / 4), or a bad device stride or alignment returns SGX_EINVAL and launches nothing; the
 * handle stays usable. */
#define SGX_EXACT_MAX_MAC 63
int sgx_exact_2bit(sgx_handle *h, const uint8_t *packed, size_t bytes_per_variant, size_t n_variants,
	const double *lut, int max_mac, double *out4);
int sgx_exact_2bit_dev(sgx_handle *h, const uint8_t *packed_dev, size_t bytes_per_variant, size_t n_variants,
	const double *lut_dev, int max_mac, double *out4_dev);

/* Pseudo-variants of groups of 2-bit rows: what SKAT and SKAT-O put in the place of a unit's ultra-rare variants
 * (saigegds_amd/aggregate.py, collapse_mac=; nothing of this is in the reference).  Group g has the entries
 * e in [grp_ptr[g], grp_ptr[g+1]) = rows var_idx[e] of `packed`, each with a byte flip[e].  An entry's minor-allele dosage
 * of sample i is its code, 2 - code where flip[e] != 0, and 0 where the code is 3 (missing).  Per group:
 *   out_rows[g]     a 2-bit row of bytes_per_variant bytes: code of sample i = the largest dosage over the group's entries
 *                   (codes 0, 1, 2 only); the fields at and beyond n_samp and the bytes beyond ceil(n_samp / 4) are 0,
 *                   whatever the input rows hold there and whatever the flips
 *   counts[2g]      samples with code 1        counts[2g + 1]   samples with code 2
 * so that out_rows is a source of sgx_scan_2bit, sgx_skat_2bit and the other entries like any row.  A group of 0 entries
 * gives an all-zero row and zero counts; a row may be in any number of groups.
 *   sgx_collapse_2bit      rows, groups and results in HOST memory; the rows cross PCIe once in the chunks of the
 *                          host-buffer scans.  Synchronous; a thin wrapper around the next entry: same kernel, same bits.
 *   sgx_collapse_2bit_dev  everything in DEVICE memory: rows and out_rows at stride and alignment of sgx_scan_2bit_dev
 *                          (out_rows at the rows' stride; the two must not overlap), grp_ptr_dev 8-byte aligned,
 *                          var_idx_dev and counts_dev 4-byte.  grp_ptr_dev and var_idx_dev are copied back and checked
 *                          first, which waits for what the handle's stream already holds; the kernel is then queued on
 *                          that stream and the results are readable after sgx_sync().
 * Integer work only (bit operations on whole words, popcounts, integer atomics for the counts): a group's row and counts
 * depend on its entries' rows and flips alone -- not on the other groups, their order, the grid or the chunks.
 * n_groups = 0 succeeds and does nothing.  A NULL buffer, grp_ptr[0] != 0 or grp_ptr not ascending, a variant index
 * outside [0, n_variants), bytes_per_variant < ceil(n_samp / 4), or a bad device stride or alignment returns SGX_EINVAL
 * and launches nothing; the handle stays usable. */
int sgx_collapse_2bit(sgx_handle *h, const uint8_t *packed, size_t bytes_per_variant, size_t n_variants, size_t n_groups,
	const int64_t *grp_ptr, const int32_t *var_idx, const uint8_t *flip, uint8_t *out_rows, int32_t *counts);
int sgx_collapse_2bit_dev(sgx_handle *h, const uint8_t *packed_dev, size_t bytes_per_variant, size_t n_variants,
	size_t n_groups, const int64_t *grp_ptr_dev, const int32_t *var_idx_dev, const uint8_t *flip_dev,
	uint8_t *out_rows_dev, int32_t *counts_dev);

/* Aggregate tests on dosage input: the INTSXP / REALSXP branches of ds_mat_mafmac and ds_mat_burden
 * (src/saige_main.cpp:485-610), which the R drivers reach with .dsnode(gdsfile, dsnode) for imputed
 * data (R/assoc_aggregate.r:89,351,606).  A batch of dosage rows (u8: 0xFF = missing; i32: INT_MIN =
 * missing; f64: NaN / Inf = missing; one row of n_samp values per variant) crosses PCIe ONCE and stays
 * on the device for the three things a driver needs from it:
 *   sgx_dsblock_create  storage for up to max_variants rows (u8: n_samp bytes a row; i32 and f64:
 *                       8 n_samp -- i32 rows are kept as doubles, as sgx_scan_i32 converts them)
 *   sgx_dsblock_load    rows in host memory -> block, in chunks of the host-buffer pipeline; returns per
 *                       variant n_valid, sum (ds_mat_mafmac's s: exact for u8 / i32, a double sum for
 *                       f64) and sum_trunc, the `int sum` of ds_mat_burden.  The reference declares that
 *                       sum `int` in the REALSXP branch too (:589-591), so it truncates after every
 *                       addition; the device returns the sum of floor(dosage), which is the same number
 *                       for finite dosages in [0, 2] with a fractional part below 1 - 2^-20.  Agreement
 *                       with the reference is claimed for dosages in that range only, and for i32 sums
 *                       (64-bit here) wherever the reference's `int` does not overflow.
 *   sgx_dsblock_scan    single-variant test of every resident row: the kernels of sgx_scan_u8 / _f64,
 *                       launched on the chunks sgx_scan_* would cut the same rows into, so rows that take
 *                       the dosage kernels there give the same results bit for bit.  Hard-call u8 / i32
 *                       rows are not packed to 2-bit here; they agree with sgx_scan_u8 / _i32 within the
 *                       scan's tolerance (integer columns exactly).
 *   sgx_dsblock_burden  n_groups units; group g has the entries [grp_ptr[g], grp_ptr[g+1]) = rows
 *                       var_idx[e] of the block, in the unit's order; n_cols weight columns per group
 *                       (1 .. SGX_DS_MAX_COLS; each pass over a group's rows feeds 8 of them).  Burden
 *                       row g * n_cols + c = sum over the group's entries with finite w[e*n_cols+c] of
 *                           present ? (flip[e] ? 2 - x : x) * w[e*n_cols+c] : mw[e*n_cols+c]
 *                       per sample, the product rounded and then added as ds_mat_burden does; the caller
 *                       forms flip (sum_trunc > n_valid) and mw = m * w, m = sum_trunc / n_valid or
 *                       2 - that (saigegds_amd/aggregate.py).  Then the single-variant test on every
 *                       row; out8 / valid: n_groups * n_cols rows.  A row of hard calls equals the row
 *                       sgx_burden_2bit makes from the packed form of the same data bit for bit.
 *   sgx_ds_block_load_packed  the load of an SGX_DS_F64 block (SGX_EINVAL for the other types) from packed-real
 *                       rows as the file stores them (raw, cls, n_file_samp, scale, offset, sel: as for
 *                       sgx_scan_packed, same checks): decoded and sample-selected on the device.  n_valid, sum,
 *                       sum_trunc and everything sgx_dsblock_scan / _burden then give equal sgx_dsblock_load of
 *                       the host-decoded rows bit for bit.  (Its name stands apart from the sgx_dsblock_* five on
 *                       purpose: that set is pinned as it is by tests/test_aggregate_dosage.py.)
 *   sgx_ds_block_skat   the SKAT sums of sgx_skat_2bit from the resident rows (named as the entry above, for the same
 *                       reason).  Unit u has the entries [unit_ptr[u], unit_ptr[u+1]) = rows var_idx[e] of the block,
 *                       in [0, rows loaded); entry e has the dosage vector
 *                           G_e(i) = present ? (flip[e] ? 2 - x : x) : mean[e],    x = row var_idx[e] at sample i
 *                       with mean[e] already flipped by the caller (the drivers: flip = sum > n_valid, mean =
 *                       sum / n_valid or 2 - that, from the double `sum` -- what the scan itself imputes and flips by;
 *                       DESIGN.md 8b).  score, cov: as sgx_skat_2bit lays them out, every unit's matrix exactly
 *                       symmetric; the same FP64 matrix-core sums in a fixed order -- no atomics, sample slabs cut by
 *                       n_samp alone, the same bits from call to call and whatever the other units of the call are.  An
 *                       entry whose mean is not finite and is used gets non-finite results and leaves the other entries
 *                       of its unit alone.  Nothing crosses PCIe but the tables and the results.  A unit of 0 entries
 *                       is legal; a unit of more than SGX_SKAT_MAX_VARIANTS entries, an index outside the loaded rows,
 *                       a NULL buffer or a block / handle mismatch returns SGX_EINVAL and launches nothing; the handle
 *                       stays usable.
 *   sgx_ds_block_cond_set  the conditional scan's sgx_cond_set for conditioning variants that are rows of a loaded
 *                       block: n_cond (0 .. SGX_COND_MAX) rows var_idx[c] with flip[c] / mean[c] as for
 *                       sgx_ds_block_skat.  score_c, cov_cc: what sgx_ds_block_skat gives for those entries as one unit,
 *                       bit for bit (the same functions).  The set lands in the handle state sgx_cond_set fills -- the
 *                       dense matrix is built on the device from the rows where they lie -- so it outlives the block's
 *                       next load and serves sgx_cond_2bit* as well; n_cond = 0 clears it.
 *   sgx_ds_block_cond   sgx_cond_2bit for all resident rows: score[j] = S_j, var[j] = Phi_jj, cov[j * n_cond + c] =
 *                       Phi_jc of the dosage vector G_j above (flip[j] / mean[j] per resident row), HOST buffers of
 *                       n_variants loaded rows.  FP64 matrix-core sums in a fixed order (Phi_jj's quadratic term on the
 *                       vector ALU): no atomics, sample slabs cut by n_samp alone, so what a row gets depends on its own
 *                       values, its flip / mean and n_samp only -- not on the number of rows, its position in the block or
 *                       the cut into launches.  A row whose mean is not finite and is used gets non-finite results and
 *                       leaves the other rows alone.  Nothing crosses PCIe but the tables and the results.
 *                       Both: a NULL buffer, nothing loaded, an index outside the loaded rows, a twin handle, a block /
 *                       handle mismatch, or sgx_ds_block_cond with no set installed returns SGX_EINVAL and launches
 *                       nothing; the handle stays usable.
 *   sgx_ds_block_firth  sgx_firth_2bit for resident rows: row r of out4 = {beta, SE, iterations, converged} of loaded row
 *                       var_idx[r] with the dosage vector G above (flip[r] / mean[r] per REQUEST; indices may repeat and
 *                       come in any order), conventions as for sgx_firth_2bit: beta for the orientation flip[r] gives, a
 *                       request whose mean is not finite {NaN, NaN, 0, 0} whether or not a sample is missing, a row
 *                       without a non-zero dosage {NaN, NaN, ., 0}.  HOST buffers of n_rows entries.  One workgroup per
 *                       request compacts the samples with G != 0 in sample order (kern_firth_ds.h) and runs the iteration
 *                       of sgx_firth_2bit on that list, FP64 sums in a fixed order, no atomics: what a request gets
 *                       depends on its row's values, its flip / mean and the model only -- not on the row's place in the
 *                       block, the request's place in var_idx, the grid or the other requests -- and a row of hard calls
 *                       gives the bits of sgx_firth_2bit on its 2-bit form with the table {0, 1, 2, mean} ({2, 1, 0, mean}
 *                       where flipped), the iteration count included.  Lists that do not fit LDS go to the scratch buffer
 *                       of sgx_firth_2bit (allocated on first use, at most 2 GiB, freed with the handle).  n_rows = 0
 *                       succeeds and does nothing.  A NULL handle, block or buffer, a twin handle, a quantitative-trait
 *                       handle, maxit < 1, nothing loaded, an index outside the loaded rows or a block / handle mismatch
 *                       returns SGX_EINVAL and launches nothing; handle and block stay usable.
 *   sgx_ds_block_collapse  the pseudo-variants of sgx_collapse_2bit for groups of resident rows (not in the
 *                       reference).  Group g has the entries [grp_ptr[g], grp_ptr[g+1]) = rows var_idx[e] of the block,
 *                       in [0, rows loaded), each with a byte flip[e]; HOST tables.  Its row holds, per sample,
 *                           top = 0;  for every entry: v = missing(x) ? 0 : (flip[e] ? 2 - x : x);  if (v > top) top = v
 *                       with x = row var_idx[e] at that sample: u8 rows in integer arithmetic (0xFF missing; a value
 *                       above 2 in a flipped row is negative and never enters), rows held as doubles (i32 and f64
 *                       blocks) with one rounded subtraction (non-finite missing; negative values, -0.0 and NaN never
 *                       enter) -- a strict maximum from +0.0, so the order of the entries and repeats change no bit, and
 *                       a group's row depends on its entries' rows and flips alone.  A row of hard calls gives the row
 *                       of sgx_collapse_2bit.  A group of 0 entries gives a row of zeros; no value of a pseudo-row is
 *                       missing.  The n_groups rows are appended to the block in its resident form (rows loaded += n_groups;
 *                       the next load resets the block) and are rows like any other to every sgx_dsblock_* /
 *                       sgx_ds_block_* entry from then on.  n_valid, sum, sum_trunc [n_groups]: what sgx_dsblock_load
 *                       returns for such rows (the same kernel); out8 [n_groups * 8], valid [n_groups]: what
 *                       sgx_dsblock_scan returns for a block of exactly these rows (the same launches); out_rows (may be
 *                       NULL): the rows themselves, n_groups * n_samp bytes (u8) or doubles.  sgx_stats after the call
 *                       are the scan's, with ms_kernel the time of the collapse kernel alone.  n_groups = 0 succeeds and
 *                       does nothing.  A NULL handle, block or buffer (but out_rows), a twin handle, nothing loaded,
 *                       grp_ptr[0] != 0 or a descending grp_ptr, an index outside the loaded rows, more rows than the
 *                       block was created for, or a block / handle mismatch returns SGX_EINVAL and launches nothing;
 *                       handle and block stay usable.
 * All of them are synchronous; block and handle must be on the same device and have the same n_samp. */
#define SGX_DS_U8  0
#define SGX_DS_I32 1
#define SGX_DS_F64 2
#define SGX_DS_MAX_COLS 64
typedef struct sgx_dsblock sgx_dsblock;
int  sgx_dsblock_create(int32_t n_samp, int dtype, size_t max_variants, int device, sgx_dsblock **out);
void sgx_dsblock_free(sgx_dsblock *b);
int  sgx_dsblock_load(sgx_handle *h, sgx_dsblock *b, const void *dosage, size_t n_variants,
	int32_t *n_valid, double *sum, int64_t *sum_trunc);
int  sgx_ds_block_load_packed(sgx_handle *h, sgx_dsblock *b, const void *raw, int cls, size_t n_file_samp,
	double scale, double offset, const int32_t *sel, size_t n_variants,
	int32_t *n_valid, double *sum, int64_t *sum_trunc);
int  sgx_ds_block_collapse(sgx_handle *h, sgx_dsblock *b, size_t n_groups, const int64_t *grp_ptr,
	const int32_t *var_idx, const uint8_t *flip, int32_t *n_valid, double *sum, int64_t *sum_trunc,
	double *out8, uint8_t *valid, void *out_rows);
int  sgx_ds_block_skat(sgx_handle *h, const sgx_dsblock *b, size_t n_units, const int64_t *unit_ptr,
	const int32_t *var_idx, const uint8_t *flip, const double *mean, double *score, double *cov);
int  sgx_ds_block_cond_set(sgx_handle *h, const sgx_dsblock *b, size_t n_cond, const int32_t *var_idx,
	const uint8_t *flip, const double *mean, double *score_c, double *cov_cc);
int  sgx_ds_block_cond(sgx_handle *h, const sgx_dsblock *b, const uint8_t *flip, const double *mean,
	double *score, double *var, double *cov);
int  sgx_ds_block_firth(sgx_handle *h, const sgx_dsblock *b, size_t n_rows, const int32_t *var_idx,
	const uint8_t *flip, const double *mean, int maxit, double *out4);
int  sgx_dsblock_scan(sgx_handle *h, const sgx_dsblock *b, double *out8, uint8_t *valid);
int  sgx_dsblock_burden(sgx_handle *h, const sgx_dsblock *b, size_t n_groups, const int64_t *grp_ptr,
	const int32_t *var_idx, const uint8_t *flip, int n_cols, const double *w, const double *mw,
	double *out8, uint8_t *valid);

/* Host-side decoder of SeqArray's genotype/data node (dBit2 [variant][sample][ploidy]) into the 2-bit dosage
 * rows of sgx_scan_2bit / sgx_block_load: code = number of non-reference alleles, 3 = missing -- SeqArray's
 * "$dosage_alt", what seqApply(.useraw=NA) hands saige_score_test_bin as RAW (R/assoc_single.r:202-221).
 * alleles: the node's bytes from the one that holds bit `bit0` (a multiple of 4) of the first wanted
 * variant; sel: sample indices to keep, in the order wanted (NULL = all n_samp); out: m rows of out_stride
 * bytes (a pinned block buffer, say).  threads: host threads to split the rows over (0 = automatic).
 * Needs no GPU. */
int sgx_decode_dbit2(const uint8_t *alleles, size_t bit0, int32_t n_samp, size_t m,
	const int64_t *sel, int32_t n_sel, uint8_t *out, size_t out_stride, int threads);

/* Per-variant counts of a HOST 2-bit matrix on GPU `device`: n_valid[j] = samples with a call,
 * allele_sum[j] = their alt-allele count -- the inputs of the maf / missing-rate variant filter of
 * seqFitNullGLMM_SPA (seqSetFilterCond, R/saige_main.r:314-321).  Needs no model handle. */
int sgx_geno_stats_2bit(const uint8_t *packed, size_t bytes_per_variant, int32_t n_samp,
	size_t n_variants, int device, int32_t *n_valid, int32_t *allele_sum);

/* GRM markers of the null-model fit from a file that holds only imputed dosages: the reference's default mode falls
 * back to annotation/format/DS and rounds every dosage to a hard call (saige_get_sparse, src/saige_fitnull.cpp:273-288;
 * R/saige_main.r:395-417).  raw: n_rows stored rows of n_file_samp values in HOST memory, cls / scale / offset / sel as
 * for sgx_scan_packed (the five SGX_PR_* classes, dosage v = raw * scale + offset in two roundings, float32 widened as
 * it is; sel: NULL or n_samp indices into the file's samples).  Per row, on GPU `device`:
 *   packed_out  ceil(n_samp/4) bytes at packed_out + row * out_stride, four samples a byte LSB first, the codes of the
 *               last byte's samples beyond n_samp 0 (bytes from ceil(n_samp/4) up to out_stride are left as they are):
 *               code 3 where v is not finite, else r = round(v) (C's round: halves away from zero) if r is 0, 1 or 2,
 *               else 3.  The range is decided in double (1e30f -> 3; -0.4 and -0.0 -> 0).  No flip to the minor allele:
 *               the orientation stays the alt allele's, as for $dosage_alt rows.
 *   n_valid, allele_sum   the codes other than 3 and their sum (the counts of sgx_geno_stats_2bit on the row)
 *   ds_valid, ds_sum      the finite dosages before rounding and their sum: for the four integer classes
 *               (double)(sum of the non-missing stored values, exact in 64 bits) * scale + ds_valid * offset, each
 *               operation rounded once; for float32 a double sum in a fixed order (a thread's 16 samples in index order,
 *               the lanes of a wave pairwise, then waves and blocks in index order).
 * All five are the same bit for bit from run to run and do not depend on chunk_bytes: the rows cross PCIe as stored in
 * chunks of chunk_bytes of raw rows (0 = 512 MiB; at least one row), chunk i + 1 uploading while chunk i is quantised
 * and its rows come back.  Needs no model handle; synchronous.  n_rows == 0 succeeds and does nothing.  A bad argument
 * (unknown cls, a NULL buffer, n_samp < 1, n_file_samp < n_samp, no sel with n_file_samp != n_samp, an index outside
 * [0, n_file_samp), out_stride < ceil(n_samp/4)) returns SGX_EINVAL, launches nothing and writes nothing. */
int sgx_quantize_packed(const void *raw, int cls, size_t n_file_samp, double scale, double offset,
	const int32_t *sel, int32_t n_samp, size_t n_rows, int device, size_t chunk_bytes,
	uint8_t *packed_out, size_t out_stride,
	int32_t *n_valid, int32_t *allele_sum, int32_t *ds_valid, double *ds_sum);

/* Pairwise LD of 2-bit rows, the kernel under seqFitLDpruning.  For rows x, y (code = alt-allele count,
 * 3 = missing) and the samples called in BOTH, six non-negative integers describe the pair:
 *     n = #both called   sx = sum x   sy = sum y   sxx = sum x^2   syy = sum y^2   sxy = sum x y
 * and with c = n sxy - sx sy, vx = n sxx - sx^2, vy = n syy - sy^2 in int64 (exact for n_samp < 2^29) the correlation is
 * r = c / sqrt(vx vy).  The pair is IN LD at t2 = t^2 iff  vx > 0 && vy > 0 && (double)c*(double)c > t2*((double)vx*(double)vy)
 * (strict: a tie is not in LD).  All sums are integer accumulations on the matrix cores: a pair's sums depend on its two
 * rows alone, and neither the 2-bit fields at and beyond n_samp in the last byte nor the bytes beyond ceil(n_samp/4)
 * enter them, whatever they hold.
 *
 * A handle needs no model.  It holds a resident BLOCK of up to SGX_LD_BLOCK candidate rows and a WINDOW of kept rows, a
 * ring that grows by doubling up to window_bytes (0 = 8 GiB).  Every entry is synchronous.  After SGX_EINVAL (a NULL
 * buffer, a row count over its cap, bytes_per_variant < ceil(n_samp/4)) or SGX_ENOMEM (the window over its budget, no
 * device memory) the handle stays usable and the window is as it was: sgx_ld_window_push changes its length and its
 * first row only once the append is done.  After SGX_EHIP (the device itself failed) the rows of the window are
 * undefined: reset it.
 *   sgx_ld_counts_2bit   host rows a[ma], b[mb] (bytes_per_variant stride, at most SGX_LD_MAX_ROWS each) ->
 *                        out[ma][mb][6] = (n, sx, sy, sxx, syy, sxy), x the row of a.  Touches neither block nor window.
 *   sgx_ld_block_2bit    uploads mb <= SGX_LD_BLOCK candidate rows as the block; flags[mb][W + mb], one byte per pair,
 *                        1 = in LD: columns 0..W-1 are the W window rows, oldest first, columns W.. the block's own
 *                        rows, of which only j < i is defined.  The sums stay on the device.
 *   sgx_ld_window_push   drops the oldest drop_oldest window rows, then appends the block's rows keep_idx[0..n_keep)
 *                        (ascending), device to device.
 *   sgx_ld_window_reset  empties the window (its memory is kept).   sgx_ld_window_len: its rows (-1: NULL handle).
 *   sgx_ld_kernel_ms     HIP-event time of the kernels of the last counts / block call. */
#define SGX_LD_BLOCK     256
#define SGX_LD_MAX_ROWS 4096
typedef struct sgx_ld sgx_ld;
int  sgx_ld_create(int device, int32_t n_samp, size_t bytes_per_variant, size_t window_bytes, sgx_ld **out);
void sgx_ld_free(sgx_ld *l);
int  sgx_ld_counts_2bit(sgx_ld *l, const uint8_t *a, size_t ma, const uint8_t *b, size_t mb, int32_t *out);
int  sgx_ld_block_2bit(sgx_ld *l, const uint8_t *rows, size_t mb, double t2, uint8_t *flags);
int  sgx_ld_window_push(sgx_ld *l, const int32_t *keep_idx, size_t n_keep, size_t drop_oldest);
int  sgx_ld_window_reset(sgx_ld *l);
int64_t sgx_ld_window_len(const sgx_ld *l);
int  sgx_ld_kernel_ms(sgx_ld *l, double *ms);

/* Tuning / test hooks (per handle; there are no process-wide switches): "spa_exact" (every flagged variant
 * through the exact exp/log SPA kernel instead of the cumulant series), "force_dense" (exact g_pos/g_neg
 * pass for every SPA variant), "score_v1" (FP64 gather score kernel instead of the MFMA path), "lanes"
 * (1..4: successive sgx_scan_block / sgx_scan_2bit_dev calls go round-robin over that many streams with
 * their own workspace, so the SPA stage of one block runs under the score stage of the next; call
 * sgx_sync() before reading any output), "pipe_mb" (MiB of input rows per chunk of a host-buffer scan;
 * 0 = default 512), "spa_scan_rows" (0 / 1: the per-variant SPA kernels scan the rows of a block instead of
 * walking its carrier lists, as they do for row-major input), "three_plane" (-1 automatic -- row-major calls take the three-plane form of the
 * contraction kernel for models of up to four B fragments (K <= 3 binary, any quantitative K <= 2) and otherwise once
 * more than ~0.5 % of the genotypes are missing, resident blocks by the census of their load; 0 / 1: never / always), "guard_exp" (x: the fixed-point guard at 10^-x instead of 2e-11; 0 = off, 300 = every
 * variant through the FP64 kernel).  Results never depend on them beyond rounding (1e-12). */
int sgx_set_option(sgx_handle *h, const char *name, long long value);

int sgx_sync(sgx_handle *h);
int sgx_get_stats(sgx_handle *h, sgx_stats *st);          /* the most recent call */
/* sums over all calls completed since the last reset (ms_* are per-stage event times: with two
 * lanes they overlap in wall time) */
int sgx_get_stats_total(sgx_handle *h, sgx_stats *st, uint64_t *n_calls, int reset);

/* Device-side helpers for the benchmark / synthetic GDS generator ---------- */

/* Smallest legal bytes_per_variant for sgx_scan_2bit_dev. */
size_t sgx_row_stride(int32_t n_samp);

/* Fill packed_dev (n_variants rows of bytes_per_variant) with synthetic 2-bit
 * genotypes: sample i of variant (first_variant+j) draws one 64-bit
 * counter-based random word (splitmix64 of seed, variant, sample); the top 32
 * bits u pick the code: u < thr[3j] -> 0, u < thr[3j+1] -> 1, else 2; the low
 * 32 bits v mark it missing when v < thr[3j+2].  thr_dev: n_variants*3 uint32
 * in device memory.  The same function in numpy: saigegds_amd/synth.py. */
int sgx_synth_2bit_dev(sgx_handle *h, uint8_t *packed_dev, size_t bytes_per_variant,
	int32_t n_samp, size_t n_variants, uint64_t first_variant, uint64_t seed,
	const uint32_t *thr_dev);

/* Null-model fit: implicit GRM on 2-bit packed genotypes ------------------------
 * The operator inside seqFitNullGLMM_SPA()'s AI-REML/PCG loop:
 *   sgx_grm_init       <- saige_store_2b_geno    src/saige_fitnull.cpp:159-230
 *   sgx_grm_diag       <- buf_diag_grm           :205-227
 *   sgx_grm_crossprod  <- get_crossprod_b_grm    :435-536   out = G'(G b)/M
 *   sgx_grm_pcg        <- PCG_diag_sigma         :581-614   (tau0 diag(1/w) + tau1 GRM) x = b
 * packed: n_markers rows of bytes_per_marker bytes, 4 samples per byte (as above);
 * vectors are host arrays of n_samp doubles. */
typedef struct sgx_grm sgx_grm;
int  sgx_grm_init(const uint8_t *packed, size_t bytes_per_marker, int32_t n_samp,
	size_t n_markers, int device, sgx_grm **out);
/* packed_dev in this GPU's HBM (copied); b_dev/out_dev device vectors */
int  sgx_grm_init_dev(const uint8_t *packed_dev, size_t bytes_per_marker, int32_t n_samp,
	size_t n_markers, int device, sgx_grm **out);
int  sgx_grm_crossprod_dev(sgx_grm *g, const double *b_dev, double *out_dev);
int  sgx_grm_sync(sgx_grm *g);
void sgx_grm_free(sgx_grm *g);
int  sgx_grm_diag(sgx_grm *g, double *diag_out);
int  sgx_grm_crossprod(sgx_grm *g, const double *b, double *out);
int  sgx_grm_pcg(sgx_grm *g, const double *w, const double *tau, const double *b,
	int maxiter, double tol, double *x_out, int *iters_out);

/* Several right-hand sides at once: the solves of one AI-REML step that share (w, tau) -- the nrun
 * Hutchinson vectors of get_trace (:627-668), Y and the columns of X in get_coeff_w (:739-758), Sigma_iX
 * and Sigma_iG of saige_GxG_snp_bin (:1477-1558) -- stream the genotypes once per iteration for all k
 * instead of once per vector.  B and Out hold k columns of N doubles, column j at B + j*ldb (a
 * row-major [k][ldb] array); Out / X use the same ldb.  1 <= k <= SGX_GRM_MAX_RHS, ldb >= N.
 *   sgx_grm_crossprod_multi(_dev)  column j = sgx_grm_crossprod(B[:, j]), bit for bit (host / device
 *                                  pointers; the _dev form is asynchronous until sgx_grm_sync)
 *   sgx_grm_pcg_multi              column j = sgx_grm_pcg(w, tau, B[:, j]): the same iterations (iters[j])
 *                                  and the same x, bit for bit; a column that meets rr <= tol or maxiter
 *                                  stops and leaves the later products; tau[1] == 0 skips the GRM
 * Scratch is allocated by the first batched call on a handle and grown to the largest k seen
 * (about 8 k N doubles, plus 96 ints per sample and per marker). */
#define SGX_GRM_MAX_RHS 64
int  sgx_grm_crossprod_multi(sgx_grm *g, const double *B, size_t ldb, int k, double *Out);
int  sgx_grm_crossprod_multi_dev(sgx_grm *g, const double *B_dev, size_t ldb, int k, double *Out_dev);
int  sgx_grm_pcg_multi(sgx_grm *g, const double *w, const double *tau, const double *B, size_t ldb, int k,
	int maxiter, double tol, double *X, int *iters);

/* Leave-one-group-out columns (LOCO: a variant of chromosome c is tested against a null model whose GRM
 * leaves out the markers of c).  A handle takes one group id per marker; column j of a *_loco call then works
 * on the GRM of the markers outside group excl[j] (-1: of all markers): G_c'(G_c b)/(M - M_c), with the
 * matching diagonal.  The packed genotypes are swept once for all columns of a call, whatever they leave out.
 *   sgx_grm_set_groups     group[n_markers]: 0 <= id < n_groups <= SGX_GRM_MAX_GROUPS, in any order (groups
 *                          need not be contiguous, and may be empty); a second call replaces the first
 *   sgx_grm_group_sizes    sizes_out[n_groups]: markers per group
 *   sgx_grm_diag_loco      diag of the GRM without group excl: (sum over the other groups, in ascending
 *                          order, of their sums of squares) / (M - M_excl); excl = -1: sgx_grm_diag
 *   sgx_grm_crossprod_loco column j = GRM_{-excl[j]} B[:, j]; with excl[j] = -1 the bits of
 *                          sgx_grm_crossprod_multi
 *   sgx_grm_pcg_loco       column j solves (tau0 diag(1/w_j) + tau1 GRM_{-excl[j]}) x = B[:, j] with
 *                          w_j = row w_idx[j] of W ([n_w][ldw], 1 <= n_w <= SGX_GRM_MAX_RHS, ldw >= N) and the
 *                          preconditioner of its own w_j and diagonal; columns run in lockstep and stop
 *                          as in sgx_grm_pcg_multi, whose bits a call with one w and excl = -1 gives
 * A column's result depends only on its own b, w and excl: not on the other columns of the call, its
 * position among them, or k.  k and ldb as above.  SGX_EINVAL: excl[j] >= 0 before sgx_grm_set_groups,
 * excl[j] >= n_groups, or a group that holds every marker (nothing is left).  Excluding an empty group is
 * excluding nothing. */
#define SGX_GRM_MAX_GROUPS 64
int  sgx_grm_set_groups(sgx_grm *g, const int32_t *group, int n_groups);
int  sgx_grm_group_sizes(sgx_grm *g, int64_t *sizes_out);
int  sgx_grm_diag_loco(sgx_grm *g, int excl, double *diag_out);
int  sgx_grm_crossprod_loco(sgx_grm *g, const double *B, size_t ldb, int k, const int *excl, double *Out);
int  sgx_grm_pcg_loco(sgx_grm *g, const double *W, size_t ldw, int n_w, const int *w_idx, const double *tau,
	const double *B, size_t ldb, int k, const int *excl, int maxiter, double tol, double *X, int *iters);

/* The explicit GRM: K = G'G/M as numbers (not in the reference, which has the operator only).
 * K_ij = (1/M) sum_v g_vi g_vj, g = fma(code, inv_v, l0_v), 0 for a missing code, summed in FP64 in marker
 * order (slabs of 65536 markers, added in slab order).  The bits of K_ij depend on the two samples' genotypes,
 * the marker table and M only: not on the rectangle, the cutoff, the other samples or the call.  K_ij and K_ji
 * are the same bits.  Marker groups (sgx_grm_set_groups) are ignored: K is always the GRM of all markers.
 *   sgx_grm_dense   out[(i - i0) * ld + (j - j0)] = K_ij, i0 <= i < i0 + ni, j0 <= j < j0 + nj: a host buffer,
 *                   any rectangle inside [0, N) x [0, N), ld >= nj; synchronous
 *   sgx_grm_sparse  every pair i <= j with K_ij >= cutoff and every diagonal entry, K_ij being the number
 *                   sgx_grm_dense gives, sorted by (i, j).  An exact int8 screen with a rigorous bound selects
 *                   the 16 x 16 sub-tiles that go to FP64; it only saves work.  *n_out is the number of entries
 *                   that exist; if it exceeds cap, SGX_ENOSPACE is returned and the buffers are not written
 *                   (call again with cap >= *n_out).  cutoff must be finite; cutoff <= -1e300 returns every
 *                   pair.  stats may be NULL.
 * SGX_EINVAL (nothing launched, nothing written): a NULL buffer, a rectangle outside [0, N), ld < nj, a
 * non-finite cutoff.  The scratch of both is allocated on first use and freed by sgx_grm_free. */
typedef struct {
	int64_t tiles_screened;      /* 64 x 64 workgroup tiles of the screen (bj >= bi)            */
	int64_t subtiles_total;      /* 16 x 16 sub-tiles with tj >= ti                             */
	int64_t subtiles_flagged;    /* those that went to FP64                                     */
	int64_t entries;             /* = *n_out                                                    */
	int32_t s;                   /* the screen quantises g to round(g 2^s)                      */
	int32_t reserved;
	double ms_prepare;           /* per-handle tables of the screen (first call only)           */
	double ms_screen, ms_fp64, ms_sort;   /* ms_fp64: tiles and compaction; ms_sort: copy and sort */
} sgx_grm_sparse_stats;
int  sgx_grm_dense(sgx_grm *g, int32_t i0, int32_t ni, int32_t j0, int32_t nj, double *out, size_t ld);
/* milliseconds the kernels of the last sgx_grm_dense call took on the device (tiles and gather; not the copy out) */
int  sgx_grm_dense_kernel_ms(sgx_grm *g, double *ms_out);
int  sgx_grm_sparse(sgx_grm *g, double cutoff, size_t cap, int32_t *i_out, int32_t *j_out, double *v_out,
	size_t *n_out, sgx_grm_sparse_stats *stats);

/* The marker side of the product, and the top principal components of K (not in the reference, which leaves PCA to
 * SNPRelate's dense N x N route).
 *   sgx_grm_marker_dots(_dev)  Out[c * ldo + v] = dot_v = sum_i G[v, i] B[i, c]: pass 1 of sgx_grm_crossprod_multi (the same
 *                   launches, so the bits the product uses internally), copied out before it becomes x_v.  B as for the
 *                   products (k columns, ldb >= N), ldo >= n_markers; host / device pointers, the _dev form asynchronous
 *                   until sgx_grm_sync.  Marker groups are ignored.  The products' results do not change by a call.
 *   sgx_grm_pca     block subspace iteration with Rayleigh-Ritz on n_block vectors from Q0 (host, [n_block][ld0]): the
 *                   block is orthonormalised by CholeskyQR twice, Y = K Q by sgx_grm_crossprod_multi_dev, H = Q'Y is
 *                   symmetrised and diagonalised by a cyclic Jacobi routine on the host, U = Q V, W = Y V,
 *                   r_c = |W_c - theta_c U_c|; it stops when r_c <= tol theta_1 for all c < n_pc or after max_iter
 *                   rounds (not an error: stats->n_converged counts the leading components that met tol), else W is the
 *                   next block.  eigval / resid [n_pc], vec [n_pc][ldv] (unit vectors, the entry of largest magnitude
 *                   positive, the lowest index on ties), loading (or NULL) [n_pc][ldl]: dot_v(U_c) / sqrt(M theta_c),
 *                   the unit left singular vector of G / sqrt(M), 0 where theta_c <= 0.  Everything N-sized stays on
 *                   the device; the bits of the outputs depend on the genotypes and on Q0 only.
 *                   SGX_ERANK (no output written, the handle stays usable): a Cholesky pivot <= n_block 2^-52 of the
 *                   largest diagonal entry -- the block's vectors are dependent, K has fewer directions than n_block.
 *                   SGX_EINVAL (nothing launched): n_pc < 1, n_block < n_pc, n_block > SGX_GRM_MAX_RHS or > N,
 *                   ld0 or ldv < N, ldl < n_markers with loading, a NULL Q0 / eigval / resid / vec, tol not finite or
 *                   < 0, max_iter < 1.
 *   sgx_grm_ts_gram / sgx_grm_ts_apply   the block kernels under the solver alone, on host arrays of any row count n
 *                   (column c at base + c * ld, ld >= n, 1 <= columns <= SGX_GRM_MAX_RHS): C[a * Lb + b] = sum_i
 *                   A[i, a] B[i, b] on the FP64 matrix cores, in slabs of SGX_TS_SLAB rows added in slab order, the bits
 *                   of C[a][b] a function of columns a, b and n only; Out[:, c] = sum_a A[:, a] T[a * Lc + c], one
 *                   fused multiply-add chain in ascending a.  Rows >= n of a column are never read or written.  For tests.
 * The scratch of all of them is allocated on first use and freed by sgx_grm_free. */
#define SGX_TS_SLAB 1024
/* af_out / inv_out [n_markers]: the allele frequency and 1 / sqrt(2 af (1 - af)) (0: monomorphic) the operator
 * standardises a marker with; what a projection of other samples onto the loadings has to repeat */
int  sgx_grm_marker_table(sgx_grm *g, double *af_out, double *inv_out);
typedef struct { int32_t iters; int32_t n_converged; double ms_products, ms_block; } sgx_grm_pca_stats;
int  sgx_grm_marker_dots(sgx_grm *g, const double *B, size_t ldb, int k, double *Out, size_t ldo);
int  sgx_grm_marker_dots_dev(sgx_grm *g, const double *B_dev, size_t ldb, int k, double *Out_dev, size_t ldo);
int  sgx_grm_pca(sgx_grm *g, int n_pc, int n_block, const double *Q0, size_t ld0, int max_iter, double tol,
	double *eigval, double *resid, double *vec, size_t ldv, double *loading, size_t ldl, sgx_grm_pca_stats *stats);
int  sgx_grm_ts_gram(sgx_grm *g, int32_t n, const double *A, size_t lda, int La, const double *B, size_t ldb, int Lb,
	double *C);
int  sgx_grm_ts_apply(sgx_grm *g, int32_t n, const double *A, size_t lda, int La, const double *T, int Lc,
	double *Out, size_t ldo);

/* KING-robust kinship of the handle's samples over its markers (not in the reference, which leaves relatedness to
 * SNPRelate's snpgdsIBDKING).  No allele frequency enters, so population structure does not inflate it.
 * Five int32 counts per pair (i, j), over the markers v < n_markers where both samples are called (code != 3):
 *     nn both called    hi code_i == 1    hj code_j == 1    hh both == 1    ibs0 codes (0, 2) or (2, 0)
 * and from them, with D = (hi + hj - 2 hh) + 4 ibs0 and mn = min(hi, hj),
 *     kinship = mn > 0 ? 0.5 - (double)D / (4.0 * (double)mn) : NaN        IBS0 = nn > 0 ? (double)ibs0 / (double)nn : NaN
 * The counts are exact (int8 matrix-core products, no floating-point sum), so a pair's five integers and the bits of
 * its kinship depend on the two samples' codes and n_markers only: not on the tile, the rectangle, the cutoff, the
 * other samples or the call; counts (j, i) are counts (i, j) with hi and hj swapped.  Marker groups are ignored.
 *   sgx_grm_king_counts  out[q * ni * ld + (i - i0) * ld + (j - j0)] = count q (0 nn, 1 hi, 2 hj, 3 hh, 4 ibs0) of the
 *                   pair (i, j), i0 <= i < i0 + ni, j0 <= j < j0 + nj: a host buffer of 5 ni ld int32, any rectangle
 *                   inside [0, N) x [0, N), ld >= nj; entries at columns >= nj of a row are not written.
 *   sgx_grm_king_pairs   every pair i < j with mn > 0 and kinship >= cutoff (a pair without a heterozygote on either
 *                   side has no kinship and is never listed), sorted by (i, j): i_out, j_out, kin_out, ibs0_out
 *                   [cap] and counts_out [cap][5] (or NULL).  *n_out is the number of pairs that exist; if it exceeds
 *                   cap, SGX_ENOSPACE is returned and the buffers are not written (call again with cap >= *n_out).
 *                   cutoff must be finite; stats may be NULL.
 * Both are synchronous.  SGX_EINVAL (nothing launched, nothing written): a NULL buffer, a rectangle outside [0, N),
 * ld < nj, a non-finite cutoff.  The scratch of both is allocated on first use and freed by sgx_grm_free. */
typedef struct {
	int64_t tiles;               /* 64 x 64 workgroup tiles contracted (bj >= bi)               */
	int64_t pairs;               /* = *n_out                                                    */
	double ms_kernel;            /* the contraction kernel on the device (HIP events)           */
	double ms_sort;              /* copy to the host and sort                                   */
} sgx_grm_king_stats;
int  sgx_grm_king_counts(sgx_grm *g, int32_t i0, int32_t ni, int32_t j0, int32_t nj, int32_t *out, size_t ld);
int  sgx_grm_king_pairs(sgx_grm *g, double cutoff, size_t cap, int32_t *i_out, int32_t *j_out, double *kin_out,
	double *ibs0_out, int32_t *counts_out, size_t *n_out, sgx_grm_king_stats *stats);

/* Operator of an explicit symmetric matrix K [n][n] resident on one device: the null-model fit on the matrix
 * sgx_grm_sparse / sgx_grm_dense made (SAIGE's useSparseGRMtoFitNULL, upstream SAIGEgds 2.x grm.mat=; not in the
 * reference, which has the implicit operator only: DESIGN.md 8f).
 *   sgx_kmat_init_csr    the full symmetric pattern (both triangles): row_ptr[n + 1] from 0, columns strictly
 *                        ascending within a row.  A row may be empty; a row without a diagonal entry has diag 0.
 *                        SGX_EINVAL: unsorted or duplicate columns, a column outside 0..n-1, a row_ptr that
 *                        decreases or does not start at 0, a non-finite value, n < 1.
 *   sgx_kmat_init_dense  row-major K with ld >= n, copied to the device; SGX_EINVAL above 8 GiB (8 n^2 bytes).
 * The other entry points follow their sgx_grm_* namesakes: host vectors, column j at B + j * ldb, Out / X with the
 * same ldb, 1 <= k <= SGX_GRM_MAX_RHS, ldb >= n, SGX_EINVAL otherwise; the _dev form takes device pointers and is
 * asynchronous until sgx_kmat_sync.  sgx_kmat_pcg_multi solves (tau[0] diag(1/w) + tau[1] K) x = b by the loop of
 * sgx_grm_pcg_multi (the same preconditioner floor, per-column scalars and exits; no product when tau[1] == 0).
 * The bits of (K b)_i depend on row i's stored entries and on b only: not on k, on the other columns of the call,
 * on the other rows or on earlier calls.  CSR rows with fewer than SGX_KMAT_WAVE_ROW entries are summed by one
 * thread in ascending column order; longer rows by a wave, lane-strided, with a fixed reduction tree.
 *   sgx_kmat_matvec_ms   milliseconds the kernels of the last product took on the device (waits for them) */
#define SGX_KMAT_WAVE_ROW 33
typedef struct sgx_kmat sgx_kmat;
int  sgx_kmat_init_csr(int32_t n, const int64_t *row_ptr, const int32_t *col, const double *val, int device,
	sgx_kmat **out);
int  sgx_kmat_init_dense(const double *K, size_t ld, int32_t n, int device, sgx_kmat **out);
void sgx_kmat_free(sgx_kmat *m);
int  sgx_kmat_sync(sgx_kmat *m);
int  sgx_kmat_diag(sgx_kmat *m, double *diag_out);
int  sgx_kmat_crossprod_multi(sgx_kmat *m, const double *B, size_t ldb, int k, double *Out);
int  sgx_kmat_crossprod_multi_dev(sgx_kmat *m, const double *B_dev, size_t ldb, int k, double *Out_dev);
int  sgx_kmat_pcg_multi(sgx_kmat *m, const double *w, const double *tau, const double *B, size_t ldb, int k,
	int maxiter, double tol, double *X_out, int *iters);
int  sgx_kmat_matvec_ms(sgx_kmat *m, double *ms_out);
/* sgx_kmat_pcg_multi on vectors that are resident on the matrix's device: w_dev [n], B_dev and X_dev at [k][ldb]
 * (they may not overlap).  The same loop on the same scalars: iterates and iters equal sgx_kmat_pcg_multi's bit for
 * bit, and column j's do not depend on k or on the other columns of the call.  Only the per-iteration scalars cross
 * to the host.  The weights cannot be checked here (the caller's: positive and finite).  Synchronous. */
int  sgx_kmat_pcg_multi_dev(sgx_kmat *m, const double *w_dev, const double *tau, const double *B_dev, size_t ldb,
	int k, int maxiter, double tol, double *X_dev, int *iters);

/* SKAT on an explicit GRM: the score statistics of sgx_skat_2bit and their covariance under the fitted model itself
 * (SAIGE-GENE's exact form; not in the reference).  Units, tables, adj_e and score[e] = S_e as for
 * sgx_skat_2bit; w [N] and tau[2] as for sgx_kmat_pcg_multi: Sigma = tau[0] diag(1/w) + tau[1] K, K the matrix of km.
 * With A the columns adj_e of a unit, X the model's covariates, Y = Sigma^-1 A (one solve per entry, in chunks of at
 * most SGX_GRM_MAX_RHS columns), Z = Sigma^-1 X (K solves per call, shared by its units), C = A'Y, D = A'Z, E = X'Z:
 *   cov, unit u (laid out as sgx_skat_2bit's):   Phi^K = 1/2 (C + C') - D E^-1 D'  =  A' P A,
 *   P = Sigma^-1 - Sigma^-1 X (X' Sigma^-1 X)^-1 X' Sigma^-1, exactly symmetric; E^-1 is made on the host in FP64.
 * No var_ratio factor: the model's own covariance needs none.  For tau[1] == 0 no product with K is made and
 * Phi^K_ef = (1 / tau[0]) sum_i w_i adj_ei adj_fi.  The solves are sgx_kmat_pcg_multi_dev's (same preconditioner floor,
 * per-column scalars and exits: a column that has not converged after maxiter steps keeps its last iterate);
 * iters[e] (may be NULL) is the step count of entry e's column.
 * Fixed order everywhere: the column sums c' and s are slab sums (slabs cut by N alone) added in slab order, so
 * score equals sgx_skat_2bit's to rounding (1e-10 relative, the scan's own bound), not bit for bit; the products run
 * in FP64 on the matrix cores over slabs of 2048 samples added in slab order, no atomics.  The bits of C_ef depend on
 * columns e and f and on N only: not on m, on the entry's position or 64-column chunk, on the other units of the
 * call or on earlier calls.  An entry whose table holds a non-finite value stays out of the solve, gets a non-finite
 * score and a non-finite row and column of its unit's cov, and leaves the other entries alone.
 * Device memory: with lda = N rounded up to 16, the call keeps 2 m lda doubles for its largest unit (A and Y), 2 K lda
 * for X and Z, and the solver's 8 min(m, 64) N; what does not fit returns SGX_ENOMEM.  The rows cross PCIe once per
 * call in the chunks of the host-buffer scans.
 * SGX_EINVAL (nothing launched, both handles stay usable): a NULL buffer, km on another device than h or of another
 * sample count, a unit above SGX_SKAT_MAX_VARIANTS, an index outside [0, n_variants), a non-finite or non-positive
 * w, tau[0] <= 0 or tau[1] < 0.  A unit of 0 entries writes nothing.  Synchronous.
 *   sgx_skat_kmat_ms   host milliseconds of the last call: ms[0] rows and columns, ms[1] solves, ms[2] products */
int sgx_skat_kmat_2bit(sgx_handle *h, sgx_kmat *km, const uint8_t *packed, size_t bytes_per_variant,
	size_t n_variants, size_t n_units, const int64_t *unit_ptr, const int32_t *var_idx,
	const double *lut, const double *w, const double *tau, int maxiter, double tol,
	double *score, double *cov, int32_t *iters /* per entry, may be NULL */);
int sgx_skat_kmat_ms(sgx_handle *h, double *ms);

/* Conditional scan on an explicit GRM: sgx_cond_set / sgx_cond_2bit with the covariances under the fitted model itself
 * (not in the reference).  Tables, adj_e, w, tau and Sigma = tau[0] diag(1/w) + tau[1] K as for
 * sgx_skat_kmat_2bit; with Phi^K as that entry defines it on the unit (c_1 .. c_C, j), the set's part is made once:
 *   sgx_cond_kmat_set   installs n_cond (1 .. SGX_COND_MAX) conditioning rows given in HOST memory: their columns A_C,
 *                       the solves Y_C = Sigma^-1 A_C and Z = Sigma^-1 X (sgx_kmat_pcg_multi_dev), E^-1 on the host.
 *                       score_c[n_cond] = S_C, cov_cc[n_cond][n_cond] = Phi^K_CC and iters_c[n_cond] (may be NULL) equal
 *                       sgx_skat_kmat_2bit on the set as one unit bit for bit.  The handle keeps A_C, Y_C, Z and X
 *                       (lda (2 n_cond + 2 K) doubles on the device, lda = n_samp rounded up to 16), D_C = A_C'Z, E^-1,
 *                       w, tau, maxiter and tol.  n_cond = 0 clears the set; a later call replaces it once everything
 *                       queued on the handle has finished.  The set is independent of sgx_cond_set's: either may be
 *                       installed, replaced or cleared without disturbing the other.
 *   sgx_cond_kmat_2bit  rows in HOST memory, uploaded in the chunks of the host-buffer scans.  Per chunk of at most
 *                       SGX_GRM_MAX_RHS rows: the adj columns, one solve of the chunk, and one kernel that makes
 *                       a_j'[Y_C | Z], A_C'y_j and a_j'y_j of every row (2 n_cond + 1 + K sums a row) with the set's
 *                       vectors shared in LDS by the chunk's row tiles; then on the host
 *                         score[j] = S_j,  var[j] = C_jj - d_j E^-1 d_j',
 *                         cov[j * n_cond + c] = 1/2 (C_jc + C_cj) - d_j E^-1 d_c'   (both orders of the last term),
 *                       iters[j] (may be NULL) the PCG steps of row j's column.  km: the matrix the set was installed
 *                       with.  score, var, cov and iters of a row equal sgx_skat_kmat_2bit's on the unit
 *                       (c_1 .. c_C, j) at the set's w, tau, maxiter and tol bit for bit: every C_ef is summed in
 *                       that entry's order (slabs of 2048 samples in slab order, no atomics), so a row's results do
 *                       not depend on the other rows, on its position or on the set installed before.
 * For tau[1] == 0 no product with K is made.  A row whose table holds a non-finite value stays out of the solve, gets
 * non-finite score, var and cov and iters = 0, and leaves the other rows alone.  n_variants = 0 succeeds and does
 * nothing.  What does not fit in device memory (besides the set: 2 x 64 lda doubles for a chunk, the solver's 8 x 64
 * n_samp) returns SGX_ENOMEM.  SGX_EINVAL (nothing launched, both handles stay usable, an installed set stays): a NULL
 * required buffer, n_cond > SGX_COND_MAX, km on another device than h or of another sample count, bytes_per_variant <
 * ceil(n_samp / 4), a non-finite or non-positive w, tau[0] <= 0 or tau[1] < 0, sgx_cond_kmat_2bit with no set installed
 * or with another km than the set's.  Both are synchronous; sgx_skat_kmat_ms gives the host milliseconds of the last
 * call of either (rows and columns, solves, products). */
int sgx_cond_kmat_set(sgx_handle *h, sgx_kmat *km, const uint8_t *packed_c, size_t bytes_per_variant, size_t n_cond,
	const double *lut_c, const double *w, const double *tau, int maxiter, double tol,
	double *score_c, double *cov_cc, int32_t *iters_c /* may be NULL */);
int sgx_cond_kmat_2bit(sgx_handle *h, sgx_kmat *km, const uint8_t *packed, size_t bytes_per_variant, size_t n_variants,
	const double *lut, double *score, double *var, double *cov /* [n_variants][n_cond] */,
	int32_t *iters /* per row, may be NULL */);

/* The three entries above on the dosage rows of a resident sgx_dsblock (imputed data; not in the reference, DESIGN.md
 * 8i).  They stand here, not beside sgx_ds_block_skat / sgx_ds_block_cond*, because they take an sgx_kmat.  Units,
 * indices and the dosage vector of an entry are sgx_ds_block_skat's,
 *     G_e(i) = present ? (flip[e] ? 2 - x : x) : mean[e],    x = row var_idx[e] at sample i
 * (u8 rows: 0xFF is missing; f64 and i32 blocks hold doubles: a non-finite value is missing; mean[e] arrives flipped);
 * w, tau, Sigma, Phi^K, the layouts, tau[1] == 0, the chunks of SGX_GRM_MAX_RHS columns, the device memory and
 * sgx_skat_kmat_ms are those of the 2-bit entries: only the kernels that make the columns adj_e and the sums c', s of
 * an entry differ.  They read a row once for all K + 1 sums, each sum in the order of the 2-bit column kernel (slabs
 * of 8192 samples cut by n_samp alone and added in slab order; in a slab thread t of 256 takes the 16-sample groups
 * t, t + 256, ... and adds a group's samples in ascending order by fma; then the block's fixed tree): no atomics, and a
 * row of hard calls gives score, cov / var and iters of its 2-bit form with the table {0, 1, 2, mean} (flipped:
 * {2, 1, 0, mean}) bit for bit.  An entry's column depends on its row, its flip / mean and n_samp only.
 *   sgx_ds_block_skat_kmat      sgx_skat_kmat_2bit for units over the loaded rows.
 *   sgx_ds_block_cond_kmat_set  sgx_cond_kmat_set for n_cond (1 .. SGX_COND_MAX) loaded rows var_idx[c].  The set lands
 *                               in the handle state sgx_cond_kmat_set fills: it outlives the block's next load and
 *                               serves sgx_cond_kmat_2bit as well; n_cond = 0 clears it (b and the buffers are not
 *                               looked at then).
 *   sgx_ds_block_cond_kmat      sgx_cond_kmat_2bit for ALL loaded rows of the block, flip[j] / mean[j] per loaded row;
 *                               HOST buffers of that many rows.  A row's results equal sgx_ds_block_skat_kmat's on the
 *                               unit (c_1 .. c_C, j) bit for bit.
 * An entry whose mean is not finite is treated like a 2-bit entry with a non-finite table -- WHETHER OR NOT a sample of
 * its row is missing (sgx_ds_block_skat looks at the mean only where it is used): its column is zeros and takes no
 * solve step, its score and its row and column of cov (var, cov of a scanned row) are non-finite at the end, its
 * iters 0, and the other entries of its unit keep their bits.
 * Nothing crosses PCIe but the entries' tables, the weights and the results.  SGX_EINVAL (nothing launched, the handles
 * stay usable, an installed set stays): a NULL handle, block or required buffer, nothing loaded, an index outside the
 * loaded rows, a unit above SGX_SKAT_MAX_VARIANTS, n_cond > SGX_COND_MAX, a twin handle, block / handle / matrix on
 * different devices or of different sample counts, a non-finite or non-positive w, tau[0] <= 0 or tau[1] < 0,
 * maxiter < 0, sgx_ds_block_cond_kmat with no set installed or with another km than the set's.  What does not fit in
 * device memory returns SGX_ENOMEM.  All three are synchronous. */
int sgx_ds_block_skat_kmat(sgx_handle *h, sgx_kmat *km, const sgx_dsblock *b, size_t n_units,
	const int64_t *unit_ptr, const int32_t *var_idx, const uint8_t *flip, const double *mean,
	const double *w, const double *tau, int maxiter, double tol,
	double *score, double *cov, int32_t *iters /* per entry, may be NULL */);
int sgx_ds_block_cond_kmat_set(sgx_handle *h, sgx_kmat *km, const sgx_dsblock *b, size_t n_cond,
	const int32_t *var_idx, const uint8_t *flip, const double *mean, const double *w, const double *tau,
	int maxiter, double tol, double *score_c, double *cov_cc, int32_t *iters_c /* may be NULL */);
int sgx_ds_block_cond_kmat(sgx_handle *h, sgx_kmat *km, const sgx_dsblock *b, const uint8_t *flip,
	const double *mean, double *score, double *var, double *cov /* [rows loaded][n_cond] */,
	int32_t *iters /* per row, may be NULL */);

/* SKAT-O: the null eigenvalues of a batch of units (saigegds_amd/skato.py; nothing of this is in the reference, DESIGN.md
 * 8k).  Problem u is a symmetric m[u] x m[u] matrix A_u = diag(w) Phi diag(w) in HOST memory; the matrices are
 * concatenated row-major as sgx_skat_2bit lays out cov (only the upper triangles are read).  One grid rho[n_rho],
 * strictly increasing within [0, 1], is shared by all problems.  With r = A 1, c = 1'A 1 (summed in a fixed order),
 * a = sqrt(1 - rho) and b = (sqrt(1 - rho + m rho) - a) / m, the n_rho + 1 matrices of a problem are
 *   k < n_rho:   B_rho[k] = R^(1/2) A R^(1/2),  R = (1 - rho) I + rho 11':   B_ij = a^2 A_ij + a b (r_i + r_j) + b^2 c
 *   k = n_rho:   W = A - r r' / c
 * (a grid of more than one value takes a value above 0.999 as 0.999; W is not clipped).
 *   eig      per problem (n_rho + 1) * m[u] doubles at (n_rho + 1) times the sum of m[v] over v < u: matrix k's
 *            eigenvalues ascending at k * m[u]
 *   sweeps   [n][n_rho + 1]: the Jacobi sweeps that rotated (0: the matrix was diagonal), at most 30
 * One workgroup per matrix runs a cyclic two-sided Jacobi iteration in FP64 (kern_eig.h): the matrix in LDS up to
 * m = 128, above that in a slice of device scratch; no eigenvectors, no atomics, a fixed order throughout, so a
 * matrix's eigenvalues have the same bits from call to call and do not depend on the other problems of the call, on
 * their order or on the other grid values; scaling A by a power of two scales them exactly.  rho = 0 iterates on A's own
 * bits.  A matrix with a non-finite entry (in A, or as formed: c = 0 for W) gets NaN eigenvalues and sweeps = -1 and
 * leaves the others alone.  n = 0 and m[u] = 0 are legal.  m[u] outside [0, SGX_SKATO_MAX_M], a bad grid or a NULL
 * buffer returns SGX_EINVAL and launches nothing; the handle stays usable.  Synchronous. */
#define SGX_SKATO_MAX_M 256
int sgx_skato_spectra(sgx_handle *h, size_t n, const int32_t *m, const double *mats, size_t n_rho,
	const double *rho, double *eig, int32_t *sweeps);

#ifdef __cplusplus
}
#endif
#endif /* SAIGEHIP_H */
