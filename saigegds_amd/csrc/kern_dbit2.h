// kern_dbit2.h -- ingest: genotype/data rows as the file stores them (dBit2 allele codes) -> 2-bit dosage rows
// Part of libsaigehip.so (single translation unit: saigehip.hip).
#pragma once

// A SeqArray file keeps hard calls as dBit2 [row][sample][ploidy]: per sample one nibble, allele a0 in bits 0-1 and a1 in
// bits 2-3, the FILE's samples in the file's order, rows back to back in one bit stream (an odd number of samples: every
// other row starts in the middle of a byte).  A site of up to three alleles is one row, a site of more takes several:
// the rows are the base-4 digits of the allele index, least significant first, all digits 3 = missing.  The dosage code
// of a sample ($dosage_alt, what sgx_decode_dbit2 and gds.py::_dosage_alt_multirow make on the host) is
//     3 if an allele is missing, else the number of alleles with a non-zero digit,
// written LSB first, four samples a byte: the rows of launch_scan<IN_2BIT> and sgx_block_load_dev.

// eight nibbles (one per sample) -> per allele, in bit 2k of the word: digit != 0, digit == 3
__device__ __forceinline__ void dbit2_digits(uint32_t w, uint32_t &nz, uint32_t &three)
{
	nz = (w | (w >> 1)) & 0x55555555u;
	three = (w & (w >> 1)) & 0x55555555u;
}

// ... -> the eight dosage codes in 16 bits.  nz / three: OR / AND of the above over the variant's rows
__device__ __forceinline__ uint32_t dbit2_codes(uint32_t nz, uint32_t three)
{
	const uint32_t alt = nz & ~three;                                    // non-reference and not missing
	const uint32_t cnt = (alt & 0x11111111u) + ((alt >> 2) & 0x11111111u);   // 0 .. 2 in each nibble
	const uint32_t miss = (three | (three >> 2)) & 0x11111111u;
	uint32_t x = cnt | miss | (miss << 1);                               // the code in bits 0-1 of each nibble
	x = (x | (x >> 2)) & 0x0F0F0F0Fu;
	x = (x | (x >> 4)) & 0x00FF00FFu;
	return (x | (x >> 8)) & 0xFFFFu;
}

__device__ __forceinline__ uint32_t dbit2_nibble(const uint8_t *__restrict__ raw, size_t nib)
{
	return ((uint32_t)raw[nib >> 1] >> ((unsigned)(nib & 1) * 4)) & 15u;
}

// the 32 samples [g0, g0 + 32) of the stored row that starts at nibble `s0` of raw, samples from n_samp on as 0:
// the two 16-byte lines of the ADDRESS that hold them, moved down by the bytes the row starts behind a line and by
// the half byte (both the same for every thread of a row: wave-uniform selects, one v_alignbit per word).  Where a
// line is not wholly inside [raw, raw + raw_bytes) -- the end of the chunk -- the nibbles are fetched one by one.
__device__ __forceinline__ void dbit2_load32(const uint8_t *__restrict__ raw, size_t raw_bytes, size_t s0, int g0, int n_samp, uint32_t d[4])
{
	const size_t nib = s0 + (size_t)g0;
	const uint8_t *p = raw + (nib >> 1);
	const unsigned a = (unsigned)(reinterpret_cast<uintptr_t>(p) & 15), sh = a * 8 + (unsigned)(nib & 1) * 4;   // bits, 0 .. 124
	const uint8_t *line = p - a;
	const int left = min(32, n_samp - g0);
	if (line >= raw && line + (sh ? 32 : 16) <= raw + raw_bytes) {
		uint32_t w[8];
		const uint4 q0 = *reinterpret_cast<const uint4 *>(line);
		w[0] = q0.x; w[1] = q0.y; w[2] = q0.z; w[3] = q0.w;
		w[4] = w[5] = w[6] = w[7] = 0;
		if (sh) {
			const uint4 q1 = *reinterpret_cast<const uint4 *>(line + 16);
			w[4] = q1.x; w[5] = q1.y; w[6] = q1.z; w[7] = q1.w;
		}
		const unsigned q = sh >> 5, r = sh & 31;
		uint32_t x[5];
#pragma unroll
		for (int i = 0; i < 5; i++) x[i] = q == 0 ? w[i] : q == 1 ? w[i + 1] : q == 2 ? w[i + 2] : w[i + 3];
#pragma unroll
		for (int i = 0; i < 4; i++) d[i] = __builtin_amdgcn_alignbit(x[i + 1], x[i], r);
		if (left < 32) {
#pragma unroll
			for (int i = 0; i < 4; i++) {
				const int keep = left - 8 * i;                          // samples of word i that exist
				d[i] = keep >= 8 ? d[i] : keep <= 0 ? 0u : d[i] & ((1u << (4 * keep)) - 1u);
			}
		}
		return;
	}
#pragma unroll
	for (int i = 0; i < 4; i++) {
		uint32_t v = 0;
		for (int k = 0; k < 8; k++)
			if (8 * i + k < left) v |= dbit2_nibble(raw, nib + 8 * i + k) << (4 * k);
		d[i] = v;
	}
}

// Row j of `out` (out_stride bytes, a multiple of 8; every byte of it is written, those beyond ceil(n_samp / 4) as 0)
// = the dosage codes of variant j.  raw: the chunk's bytes (raw_bytes of them, 16-byte aligned; nothing outside is
// read); stored row r of the chunk starts at nibble nib0 + r * n_file_samp.  row0: NULL (variant j = row j) or m + 1
// row offsets, the chunk's first row = row_base (variant j = rows row0[j] - row_base .. row0[j + 1] - row_base, at
// most 16).  Half a byte in, a quarter of a byte out per sample and row; measured at N = 430 000: 0.35 of
// the achievable HBM rate without a selection, 0.13 - 0.03 with one (the byte gathers), hidden under the chunk's copy.
// grid.x walks a row, grid.y strides over the variants.
//   sel == nullptr (n_file_samp == n_samp): a thread takes 32 samples -- 16 bytes in (dbit2_load32), 8 bytes out.
//   sel: sample i = the file's sample sel[i].  A thread makes one output dword (16 samples, as pack_rows_2bit): its 16
//     indices are read once (four 16-byte loads, consecutive threads consecutive 64 bytes) and kept for every variant
//     of its stride, the nibbles are gathered, the dword is stored coalesced.
__global__ void __launch_bounds__(256)
decode_dbit2_rows(const uint8_t *__restrict__ raw, size_t raw_bytes, unsigned nib0, size_t n_file_samp,
	const unsigned *__restrict__ row0, unsigned row_base, const int *__restrict__ sel, int n_samp, size_t m,
	uint8_t *__restrict__ out, size_t out_stride)
{
	if (sel) {
		const int nd = (int)(out_stride / 4);
		for (int dw = blockIdx.x * blockDim.x + threadIdx.x; dw < nd; dw += gridDim.x * blockDim.x) {
			int s[16];
			if (dw * 16 + 16 <= n_samp) {
#pragma unroll
				for (int k = 0; k < 4; k++) {
					const int4 v = *reinterpret_cast<const int4 *>(sel + dw * 16 + 4 * k);
					s[4 * k] = v.x; s[4 * k + 1] = v.y; s[4 * k + 2] = v.z; s[4 * k + 3] = v.w;
				}
			} else {
#pragma unroll
				for (int k = 0; k < 16; k++) s[k] = dw * 16 + k < n_samp ? sel[dw * 16 + k] : -1;
			}
			for (size_t j = blockIdx.y; j < m; j += gridDim.y) {
				const size_t ra = row0 ? row0[j] - row_base : j, rb = row0 ? row0[j + 1] - row_base : j + 1;
				uint32_t nz[2] = {0u, 0u}, three[2] = {0x55555555u, 0x55555555u};
				for (size_t r = ra; r < rb; r++) {
					const size_t s0 = (size_t)nib0 + r * n_file_samp;
					uint32_t w[2] = {0u, 0u};
#pragma unroll
					for (int k = 0; k < 16; k++)
						if (s[k] >= 0) w[k >> 3] |= dbit2_nibble(raw, s0 + (size_t)s[k]) << (4 * (k & 7));
#pragma unroll
					for (int i = 0; i < 2; i++) {
						uint32_t a, b;
						dbit2_digits(w[i], a, b);
						nz[i] |= a; three[i] &= b;
					}
				}
				// (a sample that does not exist has read no nibble: digits 0 in every row, code 0)
				reinterpret_cast<uint32_t *>(out + j * out_stride)[dw] = dbit2_codes(nz[0], three[0]) | (dbit2_codes(nz[1], three[1]) << 16);
			}
		}
		return;
	}
	const int nt = (int)(out_stride / 8);
	for (size_t j = blockIdx.y; j < m; j += gridDim.y) {
		const size_t ra = row0 ? row0[j] - row_base : j, rb = row0 ? row0[j + 1] - row_base : j + 1;
		for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < nt; t += gridDim.x * blockDim.x) {
			const int g0 = t * 32;
			uint2 o = make_uint2(0u, 0u);
			if (g0 < n_samp) {
				uint32_t nz[4] = {0u, 0u, 0u, 0u}, three[4] = {0x55555555u, 0x55555555u, 0x55555555u, 0x55555555u};
				for (size_t r = ra; r < rb; r++) {
					uint32_t d[4];
					dbit2_load32(raw, raw_bytes, (size_t)nib0 + r * n_file_samp, g0, n_samp, d);
#pragma unroll
					for (int i = 0; i < 4; i++) {
						uint32_t a, b;
						dbit2_digits(d[i], a, b);
						nz[i] |= a; three[i] &= b;
					}
				}
				o.x = dbit2_codes(nz[0], three[0]) | (dbit2_codes(nz[1], three[1]) << 16);
				o.y = dbit2_codes(nz[2], three[2]) | (dbit2_codes(nz[3], three[3]) << 16);
			}
			*reinterpret_cast<uint2 *>(out + j * out_stride + (size_t)t * 8) = o;
		}
	}
}
