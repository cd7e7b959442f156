// host_state.h -- the library's host-side state: genotype blocks and handles (lanes, workspaces, streams), on the owners of host_mem.h.
// Part of libsaigehip.so: included by saigehip.hip (one translation unit), not a header of its own.
// ---------------------------------------------------------------------------
// host side

// A block of variants: the 2-bit rows as they came (row-major: the contraction kernel's loaders read them as they
// are) with the sparse side the scan needs -- the positions of the missing genotypes and, in a resident block,
// the carrier lists of the rare variants (kern_lists.h).  Depends on the number of samples only: one block can be
// scanned with any model of that many samples.  lists_only: the scratch of the row-major scan calls -- the rows
// stay where the caller has them (ext_rows), no carrier lists.
struct sgx_block {
	int device = 0;
	int N = 0, ntile = 0, nr = 1;
	size_t cap = 0;              // variants it can hold
	size_t M = 0;                // variants loaded
	bool lists_only = false;
	// (members are released in reverse order: buffers, then events -- sgx_block_free waits for last_read first)
	DevEvent ready;              // recorded behind the last load: scans on other streams wait for it
	DevEvent last_read;          // recorded behind the last scan that reads the block: a reload waits for it
	bool was_read = false;
	DevBuf<uint8_t> rows;        // [cap][bpv] the block's copy of the rows
	size_t bpv = 0;              // bytes per row of that copy = sgx_row_stride(N)
	const uint8_t *ext_rows = nullptr; size_t ext_bpv = 0;   // lists_only: the rows of the scan in flight
	// missing genotypes (S3Lists)
	DevBuf<unsigned> idx; size_t idx_cap = 0;   // idx_cap: entries of the pool, as the kernels are told (0: no pool)
	DevBuf<unsigned> cursor;     // [S3_NSUB x S3_CURSOR_STRIDE]
	DevBuf<unsigned> lstart;     // [nr][cap]
	DevBuf<int> lcnt;            // [nr][cap]
	DevBuf<int> nzp, n2p;        // [nr][cap] non-zero codes / codes 2 per (range, variant) (resident blocks)
	DevBuf<int> n3;              // [cap] listed missing genotypes per variant
	DevBuf<uint8_t> ovf;         // [cap] 1 = not listed (the pool was full): the scan takes the FP64 kernel for it
	// carrier lists of the rare variants (at most SPA5_NNZ carriers): what the per-variant SPA kernels walk
	DevBuf<int> nzv, n2v;        // [cap] non-zero codes / codes 2 per variant (load-time scratch)
	DevBuf<unsigned> cptr;       // [cap + 1] start of a variant's list in cidx
	DevBuf<unsigned> cidx;       // sample | code << 30, ascending per variant
	size_t cidx_cap = 0;         // entries of that pool, as the kernels are told
	DevBuf<uint8_t> corient;     // [cap] 0 no list, 1 list of the non-zero codes, 2 of the codes other than 2 (AF > 0.5)
	// census of the last load (s3_lists_finish_kernel): [0] listed missing genotypes / 64, [1] variants the pool had no room for
	DevBuf<int> info; PinBuf<int> h_info;
	bool info_read = false, dense = false;
};

// The forms of the single-variant scan; scan_form picks the form of a call.
enum ScanForm {
	FORM_FP64,    // FP64 kernels: dosage rows, models the fixed-point form cannot hold, the "score_v1" hook
	FORM_LISTS,   // two planes on a resident block's lists of the missing genotypes
	FORM_ROWS,    // two planes on row-major rows, behind the fused list + T3 pass
	FORM_THREE,   // three planes: the sums over the missing samples come out of the contraction kernel, no lists
};

struct sgx_handle {
	int device = 0;
	// Members are released in reverse order of declaration: buffers, then events, then streams (sgx_free waits for the
	// streams, frees the twins and tmp_blk, then deletes).  So: streams first, events next, buffers after them.
	DevStream stream;                 // the SPA stage and everything that is not the score chain: LOW priority
	DevStream hstream;                // the score chain of a block scan (list pass, sparse pass, contraction, reduction, epilogue): HIGH priority,
	                                  // so that it is not slowed by the SPA kernels of the other lane's step it runs beside
	DevStream s3_side;                // the sparse pass over the missing genotypes (beside the list pass's tail; joined before the contraction kernel)
	DevStream cstream;                // host_pipeline.h: the copy stream, what brings a chunk into its buffers (RowSrc: src_upload)
	DevEvent s3_fork, s3_join;
	DevEvent ev[3];
	DevEvent evk[2];                  // around the contraction kernel alone (stats.ms_kernel)
	DevEvent ev_lists;                // in front of the list pass of a row-major call (stats.ms_lists = ev_lists .. ev[0])
	//  host_pipeline.h (created by ensure_pipe on first use)
	DevEvent ev_h2d;                  // scans: the chunk is in its buffers; this handle's two streams wait for it
	DevEvent ev_copy[2];              // loaders (ingest): the same per buffer; the handle's stream waits for it
	DevEvent ev_done[2];              // behind what reads a buffer on the handle's stream: the copy of the chunk after next waits for it
	// The model arrays: owned by the primary handle; md, mf[0].Fl and dQ are the views of them that every lane reads
	struct { DevBuf<double> F, X, y, mu, mu2, XM; DevBuf<uint8_t> Fl; DevBuf<long long> Q; } model;
	DevModel md{};
	// per-call workspace
	DevBuf<SpaRec> recs;             // [3 n]; the gate of ensure_recs: released first, grown last
	DevBuf<int> fallback;            // rec indices that need the exact dense pass
	DevBuf<int> fb_spa2;             // rec indices for the per-variant kernel (series on the variant's list)
	DevBuf<int> fb_x2;               // ... of those, the ones that need the exact sweeps
	int nseg = 0;                     // sample segments of the SPA stage
	bool force_dense = false;         // test hook: every SPA variant takes the exact dense pass
	// series SPA stage (kern_spa4.h)
	DevBuf<double> seg4;             // [vcap4][nseg][NC + 5] partial sums of one round of flagged variants
	int vcap4 = 0, nround4 = 0;
	bool spa5_attr_set[3] = {false, false, false};
	bool mom_attr_set[3] = {false, false, false};   // per input type: the moments kernels' dynamic LDS size has been raised
	DevBuf<uint8_t> scr5; DevBuf<int> cur5; int nwg5 = 0;   // spa5_kernel: per-workgroup lists, queue cursor
	bool spa_scan_rows = false;       // test hook: the per-variant kernels scan a block's rows instead of walking its carrier lists
	bool force_exact = false;         // test hook: every SPA variant takes the exact exp/log kernels
	// exact-integer MFMA score path (mf_fixed.h, kern_score3.h)
	bool mf_ok = false;
	MfTab mf[MF_MAXG]{};              // one limb table per column group
	int mf_nbfv[MF_MAXG]{};
	MfEpi mfe{};
	const long long *dQ = nullptr;    // [N][P] the fixed-point score values as int64 (s3_t3_kernel)
	DevBuf<int> mf_acc;
	// score3 (kern_score3.h): item slabs, partial sums over the missing samples, variants for the FP64 kernel
	DevBuf<int> s3_slabs;
	DevBuf<long long> s3_t3;
	DevBuf<int> s3_ovf;
	bool s3_attr[17] = {false};       // per NBF: dynamic LDS size raised
	bool s3_attr_miss[17] = {false};  // ... of the three-plane form
	sgx_block *tmp_blk[2] = {nullptr, nullptr};   // row-major calls: the rows are ingested into a block first
	int n_cu = 256;
	DevBuf<int> counters;            // [0] n_spa, [1] n_valid, [2] n_fallback
	PinBuf<int> h_counters;           // pinned
	DevBuf<double> scratch; size_t scratch_stride = 0; int spa_grid = 0;
	// host-pointer staging
	DevBuf<uint8_t> stage_in;
	// Host rows to the device (host_pipeline.h): chunk i + 1 crosses PCIe on the copy stream (cstream) into one buffer
	// of each pair while chunk i, in the other, is read on this handle's streams.
	size_t pipe_bytes = 0;            // "pipe_mb" option: device bytes of a chunk's rows (0 = PIPE_BYTES)
	//  the chunk's rows, by pipeline buffer
	DevBuf<uint8_t> pipe_in[2];       // as the kernels read them (copied, or decoded from pipe_raw)
	DevBuf<uint8_t> pipe_raw[2];      // as the file stores them (SRC_PACKED, SRC_DBIT2)
	DevBuf<uint8_t> pipe_pk[2];       // scans: 2-bit rows packed from hard-call u8 / i32 rows
	DevBuf<int> pipe_flag; PinBuf<int> h_pipe_flag;   // ... and whether every row of the chunk was one (pinned copy)
	//  of a call with a stored source (src_prepare)
	DevBuf<int> pk_sel;               // the sample selection
	DevBuf<unsigned> db2_row0;        // SRC_DBIT2: row offsets of the variants (multi-row sites)
	//  scans: a chunk's results on the device and in pinned host memory
	DevBuf<double> pipe_out[2]; DevBuf<uint8_t> pipe_valid[2];
	PinBuf<double> pin_out[2]; PinBuf<uint8_t> pin_valid[2];
	DevBuf<uint8_t> stage_pk;         // burden: packed rows, CSR and tables
	DevBuf<double> ds_part;           // dosage score kernels: per-split partial sums
	DevBuf<double> skat_part;         // sgx_skat_2bit: per-slab partial tiles of a launch
	DevBuf<double> skat_fin;          // ... and its tiles summed over the slabs
	DevBuf<double> stage_out; DevBuf<uint8_t> stage_valid;
	// sgx_skat_kmat_2bit (host_skat_kmat.h): a unit's adj columns and their solves [m][lda], the covariate columns and
	// theirs [2K][lda], the column sums per slab and summed, the tiles of a launch; milliseconds of the last call
	DevBuf<double> skk_A, skk_Y, skk_XZ, skk_cpart, skk_cs;
	DevBuf<SkkTile> skk_tiles;
	double skk_ms[3] = {0, 0, 0};      // columns, solve, contraction
	// conditional scan on an explicit GRM (host_cond_kmat.h): the installed set -- its vectors [A_C | Y_C | Z | X][lda],
	// what the host's last step needs of it (D_C = A_C'Z [n][K], q_C = E^-1 D_C', E^-1, rows with a non-finite table)
	// and the solve's arguments; a chunk's columns and solves are in skk_A / skk_Y
	DevBuf<double> ckm_set;
	int ckm_n = 0;                    // 0: no set installed
	sgx_kmat *ckm_km = nullptr;       // the operator the set was solved with (compared, not owned)
	std::vector<double> ckm_D, ckm_q, ckm_Einv, ckm_w;
	std::vector<uint8_t> ckm_bad;
	bool ckm_eok = false;
	double ckm_tau[2] = {0, 0}, ckm_tol = 0;
	int ckm_maxiter = 0;
	// conditional scan (host_cond.h).  Primary: the installed set -- B of kern_cond.h, the set's c' and e sums
	DevBuf<double> cond_B;
	DevBuf<double> cond_ce;           // [n_cond][2K]
	int n_cond = 0;                   // 0: no set installed
	// ... every lane: per-slab partial sums of a launch and the rows' sums over the slabs
	DevBuf<double> cond_part, cond_fin;
	// Firth effect sizes (host_firth.h): per-workgroup slices for the lists that do not fit LDS, allocated on first use
	DevBuf<uint8_t> firth_scr;
	// sgx_skato_spectra (host_skato.h): the matrices, the eigenvalues, the sweep counts, offsets and lists, and the
	// workgroups' slices of the class whose working matrix does not fit LDS
	DevBuf<double> eig_A, eig_out, eig_scr;
	DevBuf<int> eig_sw;
	DevBuf<uint8_t> eig_meta;
	bool eig_attr_set = false;
	bool evk_set = false;
	bool lists_timed = false;
	sgx_stats stats{};
	bool force_v1 = false;            // "score_v1" option: gather kernel instead of the MFMA path
	bool stats_pending = false;
	// dense g_pos / g_neg fallback of the last device-resident call, launched by the next sync if that call turned
	// out to need it (launch_spa, lazy_dense)
	struct { bool active = false; RowsRef rr{}; size_t M = 0; double *out8 = nullptr; const sgx_block *blk = nullptr; } pend_dense;
	// Lanes ("lanes" option, 1..SGX_MAX_LANES): device-resident scans go round-robin over this handle and
	// its twins, each with its own streams and workspace (the model arrays are the primary's), so that the SPA stage
	// of one block of variants runs while the score stage of the next one streams the genotypes, and -- where
	// the blocks are small (N = 50 000) -- the many short kernels of a step find others to run beside.
	// Score stages never overlap each other (the later one waits for the earlier one's event).
	sgx_handle *twins[3] = {nullptr, nullptr, nullptr};   // owned by the primary handle
	int n_lanes = 1;
	sgx_handle *owner = nullptr;      // set in a twin
	// primary: the three-plane form of the contraction kernel (no lists of the missing genotypes, cost independent of
	// the missing rate) for calls that would build lists -- set when a finished step listed more than SGX_DENSE_ON of
	// its genotypes as missing (or overflowed the pool), cleared when a three-plane step counted fewer than SGX_DENSE_OFF
	bool dense_mode = false;
	int dense_opt = -1;               // "three_plane" option: -1 automatic, 0 never, 1 always
	// bound on the z-score's move by the fixed-point columns' quantisation beyond which a variant is scored by the FP64
	// kernel (score3_epilogue): 2e-11 keeps the p-value inside 1e-10 relative with room; "guard_exp" option: 10^-x
	double guard_tol = 2e-11;
	ScanForm form = FORM_FP64;        // the form of this lane's call in flight (scan_begin; read by sync_lane)
	int next_lane = 0;                // primary: which lane takes the next _dev call
	sgx_handle *last_issued = nullptr;// primary: lane of the most recent call
	sgx_stats total{};                // primary: sums over harvested calls (sgx_get_stats_total)
	uint64_t total_calls = 0;
};

#define SGX_DENSE_ON  0.005       /* see scan_form */
#define SGX_DENSE_OFF 0.003

static int set_dev(sgx_handle *h)
{
	HIPCHK(hipSetDevice(h->device));
	return SGX_OK;
}
