// saigehip.hip -- MI355X (gfx950) kernels + C ABI of the SAIGEgds single-variant
// scan.  Interface and reference citations: include/saigehip.h; design,
// data layout and rooflines: DESIGN.md.
//
// Math of the score stage.  For a variant with (imputed, flipped) dosage G the
// reference computes (src/saige_main.cpp:300-350, either branch)
//     adj = G - X c',  c' = (X'VX)^-1 X'V G,  S = sum y_mu*adj,
//     var = r * sum mu2*adj^2.
// Both branches reduce to four carrier-only sums over I = {i : G_i != 0}:
//     c'_k = sum_I G_i A[i,k]          A = t_XVX_inv_XV
//     e_k  = sum_I G_i mu2_i X[i,k]
//     s    = sum_I G_i y_mu_i
//     w    = sum_I G_i^2 mu2_i
//     var2 = c'^T XVX c' + w - 2 e.c'        S = s - S_a.c'
// (quantitative: mu2 == 1).  The per-sample vector F[i] = [A[i,:], mu2_i X[i,:],
// y_mu_i, mu2_i] (P = 2K+2 doubles, one 16-byte aligned row) is what a carrier
// costs in memory traffic.

#include <hip/hip_runtime.h>
#include <math.h>
#include <cmath>
#include <algorithm>
#include <chrono>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <atomic>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "saigehip.h"

#define KMAX SGX_MAX_COEFF
#define WAVE 64

// ---------------------------------------------------------------------------
// error handling

static thread_local std::string g_err;

static int fail(int code, const char *fmt, ...)
{
	char buf[512];
	va_list ap;
	va_start(ap, fmt);
	vsnprintf(buf, sizeof buf, fmt, ap);
	va_end(ap);
	g_err = buf;
	return code;
}

#define HIPCHK(expr)                                                              \
	do {                                                                          \
		hipError_t e_ = (expr);                                                   \
		if (e_ != hipSuccess)                                                     \
			return fail(SGX_EHIP, "%s failed: %s (%s:%d)", #expr,                 \
				hipGetErrorString(e_), __FILE__, __LINE__);                       \
	} while (0)

#include "dev_common.h"
#include "kern_score.h"
#include "mf_fixed.h"
#include "kern_score3.h"
#include "kern_spa.h"
#include "kern_spa2.h"
#include "kern_spa4.h"
#include "kern_synth.h"
#include "kern_grm.h"
#include "kern_burden.h"
#include "kern_burden_ds.h"
#include "kern_pack.h"
#include "kern_unpack.h"
#include "kern_dbit2.h"
#include "kern_quant.h"
#include "kern_skat.h"
#include "kern_skat_ds.h"
#include "kern_cond.h"
#include "kern_cond_ds.h"
#include "kern_grm_dense.h"
#include "kern_kmat.h"
#include "kern_skat_kmat.h"
#include "kern_kmat_ds.h"
#include "kern_cond_kmat.h"
#include "kern_firth.h"
#include "kern_firth_ds.h"
#include "kern_exact.h"
#include "kern_eig.h"
#include "kern_collapse.h"
#include "kern_collapse_ds.h"
#include "kern_ld.h"
#include "kern_tsblock.h"
#include "kern_king.h"

// ---------------------------------------------------------------------------
// host side: one translation unit (every kernel template is instantiated once), in topic files
#include "host_mem.h"
#include "host_tabs.h"
#include "host_state.h"
#include "host_init.h"
#include "host_spa.h"
#include "host_lanes.h"
#include "host_blocks.h"
#include "host_scan.h"
#include "host_pipeline.h"
#include "host_rows.h"
#include "host_burden_ds.h"
#include "host_skat.h"
#include "host_skat_ds.h"
#include "host_cond.h"
#include "host_cond_ds.h"
#include "host_util.h"
#include "host_pcg.h"
#include "host_grm.h"
#include "host_grm_dense.h"
#include "host_pca.h"
#include "host_king.h"
#include "host_kmat.h"
#include "host_skat_kmat.h"
#include "host_cond_kmat.h"
#include "host_kmat_ds.h"
#include "host_firth.h"
#include "host_exact.h"
#include "host_skato.h"
#include "host_collapse.h"
#include "host_collapse_ds.h"
#include "host_ld.h"
