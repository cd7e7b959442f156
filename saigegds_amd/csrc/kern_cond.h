// kern_cond.h -- the sums of the conditional scan ("Conditional analysis"): every scanned 2-bit row
// against the 2K+1 dense columns of F and against the C conditioning variants,
//     d_j[p] = sum_i G_j(i) F[i][p],   W_jc = sum_i mu2_i G_j(i) G_c(i),   W_jj = sum_i mu2_i G_j(i)^2,
// G_j(i) = lut_j[code_ji].  The linear sums are one FP64 matrix product of the decoded rows against the dense matrix
// B [N][PB] = (F[:, 0:2K+1] | mu2 o G_c, c < C | zeros), PB = 16 NCT, built once per conditioning set; W_jj, which is
// not linear in the table, is summed on the vector ALU.  Nothing of this is in the reference.
// Part of libsaigehip.so (single translation unit: saigehip.hip).
#pragma once

#define COND_RT 4                                   // row tiles of 16 rows per wave
static const int COND_WG_ROWS = 4 * 16 * COND_RT;   // rows of a workgroup (4 waves): what one pass over B serves
static const int COND_SLAB_CH = 128;                // chunks of 256 samples per sample slab: cut by N alone

// B of a conditioning set.  One thread per (sample, column); grid.x covers N * PB.
__global__ void __launch_bounds__(256)
cond_build_kernel(const uint8_t *__restrict__ rows_c, size_t bpv, const double *__restrict__ lut_c, int n_cond,
	const double *__restrict__ F, int P, int N, int PB, double *__restrict__ B)
{
	const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
	if (t >= (size_t)N * PB) return;
	const size_t i = t / PB;
	const int p = (int)(t - i * PB), nd = P - 1;    // nd = 2K+1 dense columns
	double x = 0;
	if (p < nd) x = F[i * P + p];
	else if (p < nd + n_cond) {
		const int c = p - nd;
		const uint32_t code = (rows_c[(size_t)c * bpv + (i >> 2)] >> (2 * (i & 3))) & 3u;
		x = F[i * P + P - 1] * lut_c[4 * c + code];
	}
	B[t] = x;
}

// The lane's 16-byte piece of a row at byte o, of which only the bytes below nb may be read.
__device__ __forceinline__ uint4 cond_piece(const uint8_t *row, int o, int nb)
{
	if (o + 16 <= nb) return *reinterpret_cast<const uint4 *>(row + o);
	auto dword = [&](int k) {
		uint32_t x = 0;
#pragma unroll
		for (int b = 0; b < 4; b++)
			if (o + 4 * k + b < nb) x |= (uint32_t)row[o + 4 * k + b] << (8 * b);
		return x;
	};
	return make_uint4(dword(0), dword(1), dword(2), dword(3));
}

// grid = (row groups of COND_WG_ROWS, sample slabs of slab_ch chunks), block = 4 waves; wave w owns the COND_RT row
// tiles from row 64 w of the group on.  A chunk is 256 samples = 64 bytes of every row: lane (v = lane & 15,
// h = lane >> 4) reads bytes [16 h, 16 h + 16) of row v of each of its tiles -- four lanes per row, one 64-byte piece
// of the row's own line -- so in step t = 0..63 of the chunk its k (v_mfma_f64_16x16x4_f64: A[row v][k = h],
// B[k = h][col v], D[row h + 4 reg][col v], see kern_skat.h) is sample 256 chunk + 64 h + t.  The B fragment of a step
// (16 lanes: one 128-byte line of B per sample and column tile) is fetched once and feeds the wave's COND_RT row
// tiles; the four waves of the group read the same lines.  Samples >= N give A = B = mu2 = 0 by index and nothing is
// read for them; no byte of a row beyond ceil(N / 4) is read.  Rows >= M read row M - 1 and store nothing.  The slab's
// sums go to part[slab][row][PB + 1] (W_jj last) by plain stores: what a row gets depends on its own codes, its table
// and N alone.
template <int NCT, bool TAIL>
__device__ __forceinline__ void cond_chunk(const uint4 (&w)[COND_RT], const double (&lr)[COND_RT][4], int s0, int N,
	const double *__restrict__ F, int P, const double *__restrict__ B, int v, skat_d4 (&acc)[COND_RT][NCT], double (&wj)[COND_RT])
{
	constexpr int PB = 16 * NCT;
	uint32_t cur[COND_RT], n1[COND_RT], n2[COND_RT], n3[COND_RT];
#pragma unroll
	for (int rt = 0; rt < COND_RT; rt++) { cur[rt] = w[rt].x; n1[rt] = w[rt].y; n2[rt] = w[rt].z; n3[rt] = w[rt].w; }
#pragma unroll 1
	for (int q = 0; q < 4; q++) {
#pragma unroll
		for (int t = 0; t < 16; t++) {
			const int smp = s0 + 16 * q + t;
			const bool ok = !TAIL || smp < N;
			double m2 = 0, b[NCT];
#pragma unroll
			for (int ct = 0; ct < NCT; ct++) b[ct] = 0;
			if (ok) {
				m2 = F[(size_t)smp * P + P - 1];
				const double *bp = B + (size_t)smp * PB + v;
#pragma unroll
				for (int ct = 0; ct < NCT; ct++) b[ct] = bp[16 * ct];
			}
#pragma unroll
			for (int rt = 0; rt < COND_RT; rt++) {
				const double a = ok ? sel4(lr[rt], (cur[rt] >> (2 * t)) & 3u) : 0.0;
				wj[rt] = fma(m2 * a, a, wj[rt]);
#pragma unroll
				for (int ct = 0; ct < NCT; ct++) acc[rt][ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b[ct], acc[rt][ct], 0, 0, 0);
			}
		}
#pragma unroll
		for (int rt = 0; rt < COND_RT; rt++) { cur[rt] = n1[rt]; n1[rt] = n2[rt]; n2[rt] = n3[rt]; }
	}
}

template <int NCT>
__global__ void __launch_bounds__(256)
cond_rect_kernel(const uint8_t *__restrict__ packed, size_t bpv, int N, size_t M, const double *__restrict__ lut,
	const double *__restrict__ F, int P, const double *__restrict__ B, int slab_ch, double *__restrict__ part)
{
	constexpr int WD = 16 * NCT + 1;
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, v = lane & 15, hq = lane >> 4;
	const size_t row0 = (size_t)blockIdx.x * COND_WG_ROWS + (size_t)wave * (16 * COND_RT);
	const int nb = (N + 3) >> 2, nch = (N + 255) >> 8;
	const int c0 = blockIdx.y * slab_ch, c1 = min(nch, c0 + slab_ch);
	const uint8_t *rp[COND_RT];
	double lr[COND_RT][4], wj[COND_RT];
	skat_d4 acc[COND_RT][NCT];
#pragma unroll
	for (int rt = 0; rt < COND_RT; rt++) {
		const size_t r = min(row0 + 16 * rt + v, M - 1);
		rp[rt] = packed + r * bpv;
#pragma unroll
		for (int k = 0; k < 4; k++) lr[rt][k] = lut[4 * r + k];
		wj[rt] = 0;
#pragma unroll
		for (int ct = 0; ct < NCT; ct++) acc[rt][ct] = skat_d4{0, 0, 0, 0};
	}
	for (int ch = c0; ch < c1; ch++) {
		const int o = 64 * ch + 16 * hq, s0 = 256 * ch + 64 * hq;
		uint4 w[COND_RT];
		if (256 * ch + 256 <= N) {                  // (the same for every lane of the chunk)
#pragma unroll
			for (int rt = 0; rt < COND_RT; rt++) w[rt] = *reinterpret_cast<const uint4 *>(rp[rt] + o);
			cond_chunk<NCT, false>(w, lr, s0, N, F, P, B, v, acc, wj);
		} else {
#pragma unroll
			for (int rt = 0; rt < COND_RT; rt++) w[rt] = cond_piece(rp[rt], o, nb);
			cond_chunk<NCT, true>(w, lr, s0, N, F, P, B, v, acc, wj);
		}
	}
	double *o = part + (size_t)blockIdx.y * M * WD;
#pragma unroll
	for (int rt = 0; rt < COND_RT; rt++) {
#pragma unroll
		for (int r = 0; r < 4; r++) {
			const size_t row = row0 + 16 * rt + hq + 4 * r;
			if (row < M) {
#pragma unroll
				for (int ct = 0; ct < NCT; ct++) o[row * WD + 16 * ct + v] = acc[rt][ct][r];
			}
		}
		// W_jj: the four k-lanes of row v, added in the order of h
		const double x0 = __shfl(wj[rt], v), x1 = __shfl(wj[rt], v + 16), x2 = __shfl(wj[rt], v + 32), x3 = __shfl(wj[rt], v + 48);
		const size_t row = row0 + 16 * rt + v;
		if (hq == 0 && row < M) o[row * WD + WD - 1] = ((x0 + x1) + x2) + x3;
	}
}

// From a row's sums fin[j][WD] = (c'_j (K), e_j (K), s_j, W_jc (C), zeros, W_jj) and the conditioning variants' sums
// ce[c] = (c'_c (K), e_c (K)) to skat_finish's (host_skat.h)
//     S_j = s_j - S_a c'_j,   Phi_jl = r (c'_j XVX c'_l + W_jl - e_j c'_l - e_l c'_j),   l = j and l = each c.
// One thread per row.
__global__ void __launch_bounds__(256)
cond_finish_kernel(const double *__restrict__ fin, size_t M, int WD, DevModel md, int C, const double *__restrict__ ce,
	double *__restrict__ score, double *__restrict__ var, double *__restrict__ cov)
{
	const size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;
	if (j >= M) return;
	const int K = md.K;
	const double *cj = fin + j * WD, *ej = cj + K;
	double q[KMAX], sa = 0, cq = 0, ec = 0;
	for (int a = 0; a < K; a++) {
		double x = 0;
		for (int b = 0; b < K; b++) x += md.XVX[a * K + b] * cj[b];
		q[a] = x;
		sa += md.S_a[a] * cj[a];
	}
	const double S = cj[2 * K] - sa;
	score[j] = md.quant ? S / md.tau0 : S;
	for (int a = 0; a < K; a++) { cq += cj[a] * q[a]; ec += ej[a] * cj[a] + ej[a] * cj[a]; }
	var[j] = md.r * (cq + cj[WD - 1] - ec);
	for (int c = 0; c < C; c++) {
		const double *cl = ce + (size_t)c * 2 * K, *el = cl + K;
		cq = 0; ec = 0;
		for (int a = 0; a < K; a++) { cq += cl[a] * q[a]; ec += ej[a] * cl[a] + el[a] * cj[a]; }
		cov[j * C + c] = md.r * (cq + cj[2 * K + 1 + c] - ec);
	}
}
