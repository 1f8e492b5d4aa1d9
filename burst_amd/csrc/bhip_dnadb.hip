// burst_amd/csrc/bhip_dnadb.hip -- duplicate marks of the compressive database build (-d DNA) on the device (gfx950).
//
// The reference (process_references, DNA_16 branch, burst.c:1899-2023) bins every eligible position of a partition by its 13-mer,
// sorts each bin's windows over the symbols [13, W) and walks the runs of equal windows twice (a tally, then the marks).  Because
// the sort is lexicographic, its runs are classes of equal symbols, and the walk restates without the order:
//   24-class  = the positions of a bin with equal symbols [13, 24); full class = equal symbols [13, W);
//   a bin's last 24-class / last full class (its greatest window) is never evaluated;
//   maxChain  = max(size - 1) over the full classes that are not their bin's last;
//   maxSh     = max over bins of the sum of (size - 1) over the bin's 24-classes but the last (the tally never resets `sh`);
//   flag      = conv24 | convFull of the position's two classes.
// Here, per chunk of bins (a range of at most 2^20 bins, sized from free memory):
//   keys      (bin - first bin of the chunk) << 44 | symbols [13, 24) in 4-bit codes, radix-sorted with the position;
//             runs of equal keys are the 24-classes, runs of equal top bits the bins;
//   full      a rolling polynomial hash (mod 2^61 - 1) of the symbols [24, W) of every position, sorted inside each 24-class;
//             every run of equal hashes is checked against the symbols, and a chunk where two windows of one run differ is
//             grouped again by an exact LSD radix sort of those symbols (sixteen per 64-bit key);
//   last      the greatest window of a bin: exact lexicographic comparisons of the full classes inside the bin's last 24-class;
//   tally     the two maxima from each chunk's runs (block reductions, one atomic per block), and the two class sizes of every
//             position are kept, so that the marks -- which need the partition's thresholds -- are one pass at the end.
#include "bhip_handle.h"

namespace {

constexpr uint32_t kNL = 13;
constexpr uint32_t kStretch = 16;          // positions per thread in the count / fill passes
constexpr uint32_t kBucketShift = 16;      // bucket = bin >> 16: 1024 buckets, a chunk covers at most 16 of them (2^20 bins)
constexpr uint32_t kBuckets = 1u << (2 * kNL - kBucketShift);
constexpr uint64_t kMod = (1ull << 61) - 1;
constexpr uint32_t kHashRun = 256;         // positions per thread of the rolling hash

__device__ __forceinline__ uint64_t mulmod(uint64_t a, uint64_t b) {
	const uint64_t lo = a * b, hi = __umul64hi(a, b);
	uint64_t r = (lo & kMod) + ((lo >> 61) | (hi << 3));
	r = (r & kMod) + (r >> 61);
	return r >= kMod ? r - kMod : r;
}
__device__ __forceinline__ uint64_t addmod(uint64_t a, uint64_t b) { const uint64_t r = a + b; return r >= kMod ? r - kMod : r; }

// the reference of position p (ascending starts): the last r with start[r] <= p
__device__ __forceinline__ uint32_t ref_of(const uint64_t *start, uint32_t n, uint64_t p) {
	uint32_t lo = 0, hi = n;
	while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (start[mid] <= p) lo = mid; else hi = mid; }
	return lo;
}
// eligible (burst.c:1899-1915): a candidate of its reference (j < RefLen - W) whose first 13 symbols have codes 1..4; bin = its 13-mer
__device__ __forceinline__ bool eligible(const uint8_t *sym, const uint64_t *start, const uint32_t *len, uint32_t nref, uint32_t W,
                                         uint64_t p, uint32_t &r, uint32_t &bin) {
	while (r + 1 < nref && start[r + 1] <= p) ++r;
	if (len[r] <= W || p < start[r] || p - start[r] >= (uint64_t)(len[r] - W)) return false;
	uint32_t nib = 0;
	#pragma unroll
	for (uint32_t k = 0; k < kNL; ++k) {
		const uint32_t s = sym[p + k];
		if (s - 1u > 3u) return false;
		nib = nib << 2 | (s - 1u);
	}
	bin = nib;
	return true;
}

// rolling hash of the symbols [24, W) of every position p < n (the symbol array is padded with zeros past its end)
__global__ void k_dna_hash(const uint8_t *__restrict__ sym, uint64_t n, uint32_t L, uint64_t B, uint64_t BL1, uint64_t mask, uint64_t *__restrict__ out) {
	const uint64_t runs = (n + kHashRun - 1) / kHashRun;
	for (uint64_t t = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; t < runs; t += (uint64_t)gridDim.x * blockDim.x) {
		const uint64_t p0 = t * kHashRun, p1 = p0 + kHashRun < n ? p0 + kHashRun : n;
		const uint8_t *s = sym + 24;
		uint64_t h = 0;
		for (uint32_t k = 0; k < L; ++k) h = addmod(mulmod(h, B), (uint64_t)s[p0 + k] + 1);
		out[p0] = h & mask;
		for (uint64_t p = p0 + 1; p < p1; ++p) {
			if (L) {
				const uint64_t drop = mulmod((uint64_t)s[p - 1] + 1, BL1);
				h = addmod(mulmod(addmod(h, kMod - drop), B), (uint64_t)s[p - 1 + L] + 1);
			}
			out[p] = h & mask;
		}
	}
}

// eligible positions per bucket: a thread counts a stretch in registers while the bucket repeats (a homopolymer puts every position
// into one bin), then into the block's table in LDS, then one global add per non-empty bucket and block
__global__ void k_dna_count(const uint8_t *__restrict__ sym, uint64_t n, const uint64_t *__restrict__ start, const uint32_t *__restrict__ len,
                            uint32_t nref, uint32_t W, unsigned long long *__restrict__ counts) {
	__shared__ uint32_t hist[kBuckets];
	for (uint32_t i = threadIdx.x; i < kBuckets; i += blockDim.x) hist[i] = 0;
	__syncthreads();
	const uint64_t nstr = (n + kStretch - 1) / kStretch;
	for (uint64_t t = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; t < nstr; t += (uint64_t)gridDim.x * blockDim.x) {
		const uint64_t p0 = t * kStretch;
		uint32_t r = ref_of(start, nref, p0), cur = ~0u, c = 0, bin;
		for (uint64_t p = p0; p < p0 + kStretch && p < n; ++p) {
			if (!eligible(sym, start, len, nref, W, p, r, bin)) continue;
			const uint32_t b = bin >> kBucketShift;
			if (b != cur) { if (c) atomicAdd(&hist[cur], c); cur = b; c = 0; }
			++c;
		}
		if (c) atomicAdd(&hist[cur], c);
	}
	__syncthreads();
	for (uint32_t i = threadIdx.x; i < kBuckets; i += blockDim.x) if (hist[i]) atomicAdd(&counts[i], (unsigned long long)hist[i]);
}

// (key, position) of every eligible position whose bin lies in [bin_lo, bin_hi): block-wide compaction, one global add per tile
__global__ void __launch_bounds__(256) k_dna_fill(const uint8_t *__restrict__ sym, uint64_t n, const uint64_t *__restrict__ start,
                                                  const uint32_t *__restrict__ len, uint32_t nref, uint32_t W, uint32_t bin_lo, uint32_t bin_hi,
                                                  unsigned long long *__restrict__ counter, uint64_t cap, uint64_t *__restrict__ keys,
                                                  uint64_t *__restrict__ pos) {
	typedef hipcub::BlockScan<uint32_t, 256> Scan;
	__shared__ typename Scan::TempStorage scan_tmp;
	__shared__ unsigned long long base;
	const uint64_t tile = 256ull * kStretch, ntiles = (n + tile - 1) / tile;
	for (uint64_t tl = blockIdx.x; tl < ntiles; tl += gridDim.x) {
		const uint64_t p0 = tl * tile + (uint64_t)threadIdx.x * kStretch;
		uint32_t cnt = 0, r = p0 < n ? ref_of(start, nref, p0) : 0, bin;
		for (uint64_t p = p0; p < p0 + kStretch && p < n; ++p)
			if (eligible(sym, start, len, nref, W, p, r, bin) && bin >= bin_lo && bin < bin_hi) ++cnt;
		uint32_t off, total;
		Scan(scan_tmp).ExclusiveSum(cnt, off, total);
		if (threadIdx.x == 0) base = total ? atomicAdd(counter, (unsigned long long)total) : 0;
		__syncthreads();
		if (cnt) {
			uint64_t o = base + off;
			r = ref_of(start, nref, p0);
			for (uint64_t p = p0; p < p0 + kStretch && p < n; ++p) {
				if (!eligible(sym, start, len, nref, W, p, r, bin) || bin < bin_lo || bin >= bin_hi) continue;
				uint64_t k = (uint64_t)(bin - bin_lo);
				#pragma unroll
				for (uint32_t j = kNL; j < 24; ++j) k = k << 4 | (sym[p + j] & 15u);
				if (o < cap) { keys[o] = k; pos[o] = p; }
				++o;
			}
		}
		__syncthreads();
	}
}

// new-run flags of the sorted keys: 24-classes (whole key) and bins (the bits above 44)
__global__ void k_dna_new(const uint64_t *__restrict__ key, uint32_t m, uint32_t *__restrict__ new24, uint32_t *__restrict__ newb) {
	for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < m; i += gridDim.x * blockDim.x) {
		new24[i] = !i || key[i] != key[i - 1];
		newb[i] = !i || (key[i] >> 44) != (key[i - 1] >> 44);
	}
}
// start[id - 1] = i for each first member of a run (ids are 1-based inclusive sums of the new flags); start[runs] = m
__global__ void k_dna_starts(const uint32_t *__restrict__ nw, const uint32_t *__restrict__ id, uint32_t m, uint32_t *__restrict__ start) {
	for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < m; i += gridDim.x * blockDim.x) {
		if (nw[i]) start[id[i] - 1] = i;
		if (i == m - 1) start[id[i]] = m;
	}
}
__global__ void k_dna_gather_hash(const uint64_t *__restrict__ pos, const uint64_t *__restrict__ hash, uint32_t m, uint64_t *__restrict__ hk, uint32_t *__restrict__ idx) {
	for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < m; i += gridDim.x * blockDim.x) { hk[i] = hash[pos[i]]; idx[i] = i; }
}
__global__ void k_dna_iota(uint32_t *__restrict__ idx, uint32_t m) {
	for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < m; i += gridDim.x * blockDim.x) idx[i] = i;
}
__global__ void k_dna_gather_u32(const uint32_t *__restrict__ src, const uint32_t *__restrict__ idx, uint32_t m, uint32_t *__restrict__ out) {
	for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < m; i += gridDim.x * blockDim.x) out[i] = src[idx[i]];
}
// the exact path: 16 symbols of [24 + 16 c, 24 + 16 c + 16) (cut at W, zeros beyond) of the element idx[i], first symbol on top
__global__ void k_dna_chunk_key(const uint64_t *__restrict__ pos, const uint32_t *__restrict__ idx, const uint8_t *__restrict__ sym, uint32_t m,
                                uint32_t W, uint32_t c, uint64_t *__restrict__ out) {
	for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < m; i += gridDim.x * blockDim.x) {
		const uint8_t *s = sym + pos[idx[i]];
		uint64_t k = 0;
		#pragma unroll
		for (uint32_t j = 0; j < 16; ++j) { const uint32_t q = 24 + 16 * c + j; k = k << 4 | (q < W ? (uint64_t)(s[q] & 15u) : 0ull); }
		out[i] = k;
	}
}

// lexicographic comparison of the windows [24, W) at a and b by one wave: <0, 0, >0
__device__ __forceinline__ int wave_cmp(const uint8_t *sym, uint64_t a, uint64_t b, uint32_t L) {
	const uint32_t lane = threadIdx.x & 63;
	for (uint32_t k = 0; k < L; k += 64) {
		const uint32_t q = k + lane;
		const int x = q < L ? sym[a + 24 + q] : 0, y = q < L ? sym[b + 24 + q] : 0;
		const unsigned long long d = __ballot(x != y);
		if (d) {
			const int first = __ffsll((long long)d) - 1;
			const int dx = __shfl(x - y, first);
			return dx;
		}
	}
	return 0;
}

// full-class boundaries in the order ord (sorted by 24-class, then hash or symbols): new when the 24-class changes, or (hash mode) the
// hash, or (exact mode) the symbols.  Hash mode marks the equal-hash neighbours for the exact check (k_dna_verify).
__global__ void k_dna_newf(const uint32_t *__restrict__ ord, const uint32_t *__restrict__ id24, const uint64_t *__restrict__ pos,
                           const uint64_t *__restrict__ hash, uint32_t m, uint32_t *__restrict__ newf, uint8_t *__restrict__ check) {
	for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < m; j += gridDim.x * blockDim.x) {
		uint32_t nw = 1; uint8_t ck = 0;
		if (j && id24[j] == id24[j - 1]) {
			if (hash) { nw = hash[pos[ord[j]]] != hash[pos[ord[j - 1]]]; ck = !nw; }
			else { nw = 0; ck = 1; }      // exact mode: the symbols decide (k_dna_verify writes newf)
		}
		newf[j] = nw; check[j] = ck;
	}
}
// one wave per marked neighbour pair: hash mode -> a difference is a collision; exact mode -> a difference starts a new class
__global__ void k_dna_verify(const uint32_t *__restrict__ ord, const uint64_t *__restrict__ pos, const uint8_t *__restrict__ sym, uint32_t m,
                             uint32_t L, const uint8_t *__restrict__ check, int exact, uint32_t *__restrict__ newf, uint32_t *__restrict__ collided) {
	const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = (gridDim.x * blockDim.x) >> 6;
	for (uint32_t j = wave; j < m; j += nwaves) {
		if (!check[j]) continue;
		const int d = wave_cmp(sym, pos[ord[j - 1]], pos[ord[j]], L);
		if (d && (threadIdx.x & 63) == 0) {
			if (exact) newf[j] = 1;
			else *collided = 1;
		}
	}
}
// the greatest full class of every bin (it lies in the bin's last 24-class): one wave per bin
__global__ void k_dna_last_full(const uint32_t *__restrict__ startB, uint32_t nb, const uint32_t *__restrict__ id24, const uint32_t *__restrict__ start24,
                                const uint32_t *__restrict__ idF, const uint32_t *__restrict__ startF, const uint32_t *__restrict__ ord,
                                const uint64_t *__restrict__ pos, const uint8_t *__restrict__ sym, uint32_t L, int exact, uint32_t *__restrict__ lastF) {
	const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = (gridDim.x * blockDim.x) >> 6;
	for (uint32_t b = wave; b < nb; b += nwaves) {
		const uint32_t e = startB[b + 1], s = start24[id24[e - 1] - 1];
		const uint32_t f0 = idF[s] - 1, f1 = idF[e - 1] - 1;
		uint32_t best = f1;
		if (!exact && f1 > f0) {
			best = f0;
			for (uint32_t f = f0 + 1; f <= f1; ++f)
				if (wave_cmp(sym, pos[ord[startF[f]]], pos[ord[startF[best]]], L) > 0) best = f;
		}
		if ((threadIdx.x & 63) == 0) lastF[b] = best;
	}
}
// the two class sizes of every position (minus one; 0 for a bin's last class) and the chunk's tally: max over full classes, and
// per bin (at its last element) the sum of (size - 1) over its 24-classes but the last = members before the last 24-class minus the
// number of 24-classes before it
__global__ void __launch_bounds__(256) k_dna_tally(const uint32_t *__restrict__ ord, const uint64_t *__restrict__ pos, uint32_t m,
                                                   const uint32_t *__restrict__ id24, const uint32_t *__restrict__ start24,
                                                   const uint32_t *__restrict__ idB, const uint32_t *__restrict__ startB,
                                                   const uint32_t *__restrict__ idF, const uint32_t *__restrict__ startF,
                                                   const uint32_t *__restrict__ lastF, uint64_t *__restrict__ cls, unsigned long long *__restrict__ maxima) {
	__shared__ unsigned long long red[2][4];
	unsigned long long mc = 0, ms = 0;
	for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < m; j += gridDim.x * blockDim.x) {
		const uint32_t b = idB[j] - 1, c = id24[j] - 1, f = idF[j] - 1;
		const uint32_t s24 = start24[c], e24 = start24[c + 1], sb = startB[b], eb = startB[b + 1];
		const uint32_t c24 = e24 != eb ? e24 - s24 - 1 : 0;
		const uint32_t cf = f != lastF[b] ? startF[f + 1] - startF[f] - 1 : 0;
		cls[pos[ord[j]]] = (uint64_t)c24 | (uint64_t)cf << 32;
		if (cf > mc) mc = cf;
		if (j == eb - 1) { const unsigned long long v = (unsigned long long)(s24 - sb) - (id24[j] - id24[sb]); if (v > ms) ms = v; }
	}
	for (int o = 32; o; o >>= 1) { const unsigned long long a = __shfl_xor(mc, o), b2 = __shfl_xor(ms, o); mc = a > mc ? a : mc; ms = b2 > ms ? b2 : ms; }
	if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = mc; red[1][threadIdx.x >> 6] = ms; }
	__syncthreads();
	if (threadIdx.x == 0) {
		for (int w = 1; w < (int)(blockDim.x >> 6); ++w) { if (red[0][w] > mc) mc = red[0][w]; if (red[1][w] > ms) ms = red[1][w]; }
		if (mc) atomicMax(&maxima[0], mc);
		if (ms) atomicMax(&maxima[1], ms);
	}
}
// the marks (burst.c:1993-2023) from the two class sizes and the partition's thresholds
__global__ void k_dna_mark(const uint64_t *__restrict__ cls, uint64_t n, uint64_t sh1, uint64_t sh2, uint64_t sh3, uint64_t maxChain, uint8_t *__restrict__ flags) {
	for (uint64_t p = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; p < n; p += (uint64_t)gridDim.x * blockDim.x) {
		const uint64_t v = cls[p], c24 = (uint32_t)v, cf = v >> 32;
		uint8_t f = 0;
		if (c24 > sh1) f = c24 >= sh3 ? 3 : c24 >= sh2 ? 2 : 1;
		if (cf && maxChain) {
			uint64_t t = cf * 2048 / maxChain;
			if (t > 2048) t = 2048;
			f |= t ? (uint8_t)(31 - __clz((uint32_t)t) + 4) : 3;      // t == 0: the compiled reference's 35 - lzcnt(0) (bh_dna.c)
		}
		flags[p] = f;
	}
}

struct DnaBuf : DBuf {
	~DnaBuf() { release(); }
	template <typename T> T *as() const { return (T *)p; }
};

inline uint64_t powmod_host(uint64_t b, uint64_t e) {
	auto mul = [](uint64_t a, uint64_t c) { const unsigned __int128 x = (unsigned __int128)a * c; uint64_t r = (uint64_t)(x & kMod) + (uint64_t)(x >> 61); r = (r & kMod) + (r >> 61); return r >= kMod ? r - kMod : r; };
	uint64_t r = 1;
	for (; e; e >>= 1, b = mul(b, b)) if (e & 1) r = mul(r, b);
	return r;
}
inline uint32_t grid_for(uint64_t n, uint32_t block = 256, uint32_t cap = 8192) { const uint64_t g = (n + block - 1) / block; return (uint32_t)(g < 1 ? 1 : g > cap ? cap : g); }

}  // namespace

#define DCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return fail(BHIP_E_DEVICE, "%s:%d %s: %s", __FILE__, __LINE__, #x, hipGetErrorString(e_)); } while (0)
#define DRES(buf, bytes) do { if ((buf).reserve_exact(bytes)) return BHIP_E_DEVICE; peak += (buf).cap; } while (0)

extern "C" int bhip_dna_marks(int device, const uint8_t *sym, uint64_t sym_len, const uint64_t *ref_start, const uint32_t *ref_len,
                          uint64_t n_refs, uint32_t W, uint64_t *max_chain, uint64_t *max_sh, uint8_t *flags, uint64_t *info) {
	if (!sym || !ref_start || !ref_len || !max_chain || !max_sh || !flags) return fail(BHIP_E_ARG, "null argument");
	if (W < 24) return fail(BHIP_E_ARG, "window %u (shear + overlap) below 24 symbols", W);
	if (!n_refs || n_refs >= 0xFFFFFFFFull) return fail(BHIP_E_ARG, "%llu references", (unsigned long long)n_refs);
	for (uint64_t i = 0; i < n_refs; ++i)
		if ((i && ref_start[i] < ref_start[i - 1] + ref_len[i - 1]) || ref_start[i] + ref_len[i] > sym_len) return fail(BHIP_E_ARG, "reference %llu outside the symbols", (unsigned long long)i);
	int n_dev = 0;
	if (hipGetDeviceCount(&n_dev) != hipSuccess || device < 0 || device >= n_dev) { (void)hipGetLastError(); return fail(BHIP_E_DEVICE, "no such device"); }
	DCHK(hipSetDevice(device));
	const uint32_t nref = (uint32_t)n_refs, L = W - 24;
	const bool dbg = getenv("BHIP_DEBUG") != nullptr;
	using clk = std::chrono::steady_clock;
	auto t0 = clk::now();
	double us_up = 0, us_sort = 0, us_cls = 0, us_mark = 0;
	auto lap = [&](double &acc) { (void)hipDeviceSynchronize(); const auto t = clk::now(); acc += std::chrono::duration<double, std::micro>(t - t0).count(); t0 = t; };
	uint64_t peak = 0;
	DnaBuf d_sym, d_start, d_len, d_hash, d_cls, d_flags, d_counts, d_misc;
	// the symbols, padded with zeros for the windows and hashes that run past the end
	DRES(d_sym, sym_len + W + 64);
	DCHK(hipMemset(d_sym.p, 0, sym_len + W + 64));
	DCHK(hipMemcpy(d_sym.p, sym, sym_len, hipMemcpyHostToDevice));
	DRES(d_start, n_refs * 8); DRES(d_len, n_refs * 4);
	DCHK(hipMemcpy(d_start.p, ref_start, n_refs * 8, hipMemcpyHostToDevice));
	DCHK(hipMemcpy(d_len.p, ref_len, n_refs * 4, hipMemcpyHostToDevice));
	lap(us_up);
	DRES(d_hash, sym_len * 8 + 8); DRES(d_cls, sym_len * 8 + 8); DRES(d_counts, kBuckets * 8 + 64); DRES(d_misc, 64);
	DCHK(hipMemset(d_cls.p, 0, sym_len * 8 + 8));
	DCHK(hipMemset(d_counts.p, 0, kBuckets * 8 + 64));
	// test hook: a hash of two bits, so that the exact path runs
	const uint64_t mask = getenv("BURST_DNA_WEAK_HASH") ? 3ull : ~0ull;
	const uint64_t B = 0x1F3D5B79A3C1ull % kMod, BL1 = L ? powmod_host(B, L - 1) : 0;
	hipLaunchKernelGGL(k_dna_hash, dim3(grid_for((sym_len + kHashRun - 1) / kHashRun, 256, 65535)), dim3(256), 0, 0, d_sym.as<uint8_t>(), sym_len, L, B, BL1, mask, d_hash.as<uint64_t>());
	hipLaunchKernelGGL(k_dna_count, dim3(grid_for((sym_len + kStretch - 1) / kStretch, 256, 2048)), dim3(256), 0, 0, d_sym.as<uint8_t>(), sym_len,
	                   d_start.as<uint64_t>(), d_len.as<uint32_t>(), nref, W, d_counts.as<unsigned long long>());
	DCHK(hipGetLastError());
	std::vector<unsigned long long> counts(kBuckets);
	DCHK(hipMemcpy(counts.data(), d_counts.p, kBuckets * 8, hipMemcpyDeviceToHost));
	lap(us_cls);
	uint64_t eligible = 0, max_bucket = 0;
	for (uint64_t c : counts) { eligible += c; if (c > max_bucket) max_bucket = c; }
	if (max_bucket >= 0x7FFFFFFFull) return fail(BHIP_E_DEVICE, "one 2^16-bin bucket holds %llu positions (at most 2^31 - 1): use more partitions (-dp)", (unsigned long long)max_bucket);
	// chunks: consecutive buckets while the elements fit the memory budget (about 100 bytes each) and the bin range 2^20
	size_t free_b = 0, total_b = 0;
	DCHK(hipMemGetInfo(&free_b, &total_b));
	uint64_t budget = (uint64_t)(free_b * 0.6) / 100;
	if (budget > 0x7FFFFFFEull) budget = 0x7FFFFFFEull;
	if (const char *ev = getenv("BURST_DNA_CHUNK")) { const uint64_t f = strtoull(ev, nullptr, 10); if (f && f < budget) budget = f; }
	std::vector<std::pair<uint32_t, uint32_t>> chunks;
	uint64_t chunk_max = 0;
	for (uint32_t b = 0; b < kBuckets;) {
		uint32_t e = b; uint64_t s = 0;
		while (e < kBuckets && e - b < 16 && (e == b || s + counts[e] <= budget)) s += counts[e++];
		if (s) { chunks.push_back({b, e}); if (s > chunk_max) chunk_max = s; }
		b = e;
	}
	const uint32_t M = (uint32_t)chunk_max;
	DnaBuf k0, k1, p0, p1, i0, i1, u0, u1, id24, idB, idF, s24, sB, sF, nw24, nwB, nwF, chk, lastF, tmp;
	uint64_t exact_chunks = 0;
	unsigned long long tallies[2] = {0, 0};
	if (M) {
		DRES(k0, (size_t)M * 8); DRES(k1, (size_t)M * 8); DRES(p0, (size_t)M * 8); DRES(p1, (size_t)M * 8);
		DRES(i0, (size_t)M * 4); DRES(i1, (size_t)M * 4); DRES(u0, (size_t)M * 4); DRES(u1, (size_t)M * 4);
		DRES(id24, (size_t)M * 4); DRES(idB, (size_t)M * 4); DRES(idF, (size_t)M * 4);
		DRES(s24, (size_t)M * 4 + 8); DRES(sB, (size_t)M * 4 + 8); DRES(sF, (size_t)M * 4 + 8);
		DRES(nw24, (size_t)M * 4); DRES(nwB, (size_t)M * 4); DRES(nwF, (size_t)M * 4); DRES(chk, (size_t)M); DRES(lastF, (size_t)M * 4 + 8);
		size_t tb = 0, t1 = 0;
		{
			hipcub::DoubleBuffer<uint64_t> kk(k0.as<uint64_t>(), k1.as<uint64_t>()), pp(p0.as<uint64_t>(), p1.as<uint64_t>());
			hipcub::DoubleBuffer<uint32_t> ii(i0.as<uint32_t>(), i1.as<uint32_t>()), uu(u0.as<uint32_t>(), u1.as<uint32_t>());
			DCHK(hipcub::DeviceRadixSort::SortPairs(nullptr, t1, kk, pp, (int)M, 0, 64)); tb = std::max(tb, t1);
			DCHK(hipcub::DeviceRadixSort::SortPairs(nullptr, t1, kk, ii, (int)M, 0, 64)); tb = std::max(tb, t1);
			DCHK(hipcub::DeviceRadixSort::SortPairs(nullptr, t1, uu, ii, (int)M, 0, 32)); tb = std::max(tb, t1);
			DCHK(hipcub::DeviceScan::InclusiveSum(nullptr, t1, u0.as<uint32_t>(), u1.as<uint32_t>(), (int)M)); tb = std::max(tb, t1);
		}
		DRES(tmp, tb + 256);
	}
	unsigned long long *d_ctr = d_misc.as<unsigned long long>();     // [0] fill counter, [1] maxChain, [2] maxSh, [3] collision
	DCHK(hipMemset(d_misc.p, 0, 64));
	for (const auto &ch : chunks) {
		const uint32_t bin_lo = ch.first << kBucketShift, bin_hi = ch.second << kBucketShift;
		uint64_t m64 = 0;
		for (uint32_t b = ch.first; b < ch.second; ++b) m64 += counts[b];
		const uint32_t m = (uint32_t)m64;
		DCHK(hipMemset(d_ctr, 0, 8));
		hipLaunchKernelGGL(k_dna_fill, dim3(grid_for((sym_len + 256 * kStretch - 1) / (256 * kStretch), 1, 4096)), dim3(256), 0, 0, d_sym.as<uint8_t>(), sym_len,
		                   d_start.as<uint64_t>(), d_len.as<uint32_t>(), nref, W, bin_lo, bin_hi, d_ctr, (uint64_t)m, k0.as<uint64_t>(), p0.as<uint64_t>());
		DCHK(hipGetLastError());
		unsigned long long filled = 0;
		DCHK(hipMemcpy(&filled, d_ctr, 8, hipMemcpyDeviceToHost));
		if (filled != m) return fail(BHIP_E_INTERNAL, "chunk [%u, %u): %llu positions filled, %u counted", bin_lo, bin_hi, filled, m);
		int end_bit = 44; while ((1u << (end_bit - 44)) < bin_hi - bin_lo) ++end_bit;
		hipcub::DoubleBuffer<uint64_t> kk(k0.as<uint64_t>(), k1.as<uint64_t>()), pp(p0.as<uint64_t>(), p1.as<uint64_t>());
		size_t tbytes = tmp.cap;
		DCHK(hipcub::DeviceRadixSort::SortPairs(tmp.p, tbytes, kk, pp, (int)m, 0, end_bit));
		const uint64_t *key = kk.Current(), *pos = pp.Current();
		lap(us_sort);
		const uint32_t g = grid_for(m);
		hipLaunchKernelGGL(k_dna_new, dim3(g), dim3(256), 0, 0, key, m, nw24.as<uint32_t>(), nwB.as<uint32_t>());
		tbytes = tmp.cap; DCHK(hipcub::DeviceScan::InclusiveSum(tmp.p, tbytes, nw24.as<uint32_t>(), id24.as<uint32_t>(), (int)m));
		tbytes = tmp.cap; DCHK(hipcub::DeviceScan::InclusiveSum(tmp.p, tbytes, nwB.as<uint32_t>(), idB.as<uint32_t>(), (int)m));
		hipLaunchKernelGGL(k_dna_starts, dim3(g), dim3(256), 0, 0, nw24.as<uint32_t>(), id24.as<uint32_t>(), m, s24.as<uint32_t>());
		hipLaunchKernelGGL(k_dna_starts, dim3(g), dim3(256), 0, 0, nwB.as<uint32_t>(), idB.as<uint32_t>(), m, sB.as<uint32_t>());
		// full classes: sort inside each 24-class by hash (LSD: hash, then the class id, both stable) -- the permutation stays inside
		// the 24-classes, so their runs (and the bins') are the same slots in both orders
		// (the keys are spent once the run flags exist: their two buffers take the hashes)
		hipcub::DoubleBuffer<uint64_t> hkb(k0.as<uint64_t>(), k1.as<uint64_t>());
		hipcub::DoubleBuffer<uint32_t> ii(i0.as<uint32_t>(), i1.as<uint32_t>()), uu(u0.as<uint32_t>(), u1.as<uint32_t>());
		hipLaunchKernelGGL(k_dna_gather_hash, dim3(g), dim3(256), 0, 0, pos, d_hash.as<uint64_t>(), m, hkb.Current(), ii.Current());
		tbytes = tmp.cap; DCHK(hipcub::DeviceRadixSort::SortPairs(tmp.p, tbytes, hkb, ii, (int)m, 0, mask == ~0ull ? 64 : 2));
		hipLaunchKernelGGL(k_dna_gather_u32, dim3(g), dim3(256), 0, 0, id24.as<uint32_t>(), ii.Current(), m, uu.Current());
		tbytes = tmp.cap; DCHK(hipcub::DeviceRadixSort::SortPairs(tmp.p, tbytes, uu, ii, (int)m, 0, 32));
		const uint32_t *ord = ii.Current();
		const uint32_t vgrid = grid_for((uint64_t)m * 64, 256, 16384);
		DCHK(hipMemset(d_ctr + 3, 0, 8));
		hipLaunchKernelGGL(k_dna_newf, dim3(g), dim3(256), 0, 0, ord, id24.as<uint32_t>(), pos, d_hash.as<uint64_t>(), m, nwF.as<uint32_t>(), chk.as<uint8_t>());
		hipLaunchKernelGGL(k_dna_verify, dim3(vgrid), dim3(256), 0, 0, ord, pos, d_sym.as<uint8_t>(), m, L, chk.as<uint8_t>(), 0, nwF.as<uint32_t>(), (uint32_t *)(d_ctr + 3));
		DCHK(hipGetLastError());
		unsigned long long collided = 0;
		DCHK(hipMemcpy(&collided, d_ctr + 3, 8, hipMemcpyDeviceToHost));
		int exact = 0;
		if (collided) {
			// two different windows share a hash inside a 24-class: this chunk's full classes come from an exact LSD radix sort of the
			// symbols [24, W), sixteen per pass from the last, then the 24-class id (all passes stable)
			exact = 1; ++exact_chunks;
			hipLaunchKernelGGL(k_dna_iota, dim3(g), dim3(256), 0, 0, ii.Current(), m);
			for (uint32_t c = (L + 15) / 16; c-- > 0;) {
				hipLaunchKernelGGL(k_dna_chunk_key, dim3(g), dim3(256), 0, 0, pos, ii.Current(), d_sym.as<uint8_t>(), m, W, c, hkb.Current());
				tbytes = tmp.cap; DCHK(hipcub::DeviceRadixSort::SortPairs(tmp.p, tbytes, hkb, ii, (int)m, 0, 64));
			}
			hipLaunchKernelGGL(k_dna_gather_u32, dim3(g), dim3(256), 0, 0, id24.as<uint32_t>(), ii.Current(), m, uu.Current());
			tbytes = tmp.cap; DCHK(hipcub::DeviceRadixSort::SortPairs(tmp.p, tbytes, uu, ii, (int)m, 0, 32));
			ord = ii.Current();
			hipLaunchKernelGGL(k_dna_newf, dim3(g), dim3(256), 0, 0, ord, id24.as<uint32_t>(), pos, (const uint64_t *)nullptr, m, nwF.as<uint32_t>(), chk.as<uint8_t>());
			hipLaunchKernelGGL(k_dna_verify, dim3(vgrid), dim3(256), 0, 0, ord, pos, d_sym.as<uint8_t>(), m, L, chk.as<uint8_t>(), 1, nwF.as<uint32_t>(), (uint32_t *)(d_ctr + 3));
			if (dbg) fprintf(stderr, "[bhip] dna marks: hash collision in bins [%u, %u): exact grouping\n", bin_lo, bin_hi);
		}
		tbytes = tmp.cap; DCHK(hipcub::DeviceScan::InclusiveSum(tmp.p, tbytes, nwF.as<uint32_t>(), idF.as<uint32_t>(), (int)m));
		hipLaunchKernelGGL(k_dna_starts, dim3(g), dim3(256), 0, 0, nwF.as<uint32_t>(), idF.as<uint32_t>(), m, sF.as<uint32_t>());
		uint32_t nb = 0;
		DCHK(hipMemcpy(&nb, idB.as<uint32_t>() + (m - 1), 4, hipMemcpyDeviceToHost));
		hipLaunchKernelGGL(k_dna_last_full, dim3(grid_for((uint64_t)nb * 64, 256, 16384)), dim3(256), 0, 0, sB.as<uint32_t>(), nb, id24.as<uint32_t>(), s24.as<uint32_t>(),
		                   idF.as<uint32_t>(), sF.as<uint32_t>(), ord, pos, d_sym.as<uint8_t>(), L, exact, lastF.as<uint32_t>());
		hipLaunchKernelGGL(k_dna_tally, dim3(g), dim3(256), 0, 0, ord, pos, m, id24.as<uint32_t>(), s24.as<uint32_t>(), idB.as<uint32_t>(), sB.as<uint32_t>(),
		                   idF.as<uint32_t>(), sF.as<uint32_t>(), lastF.as<uint32_t>(), d_cls.as<uint64_t>(), d_ctr + 1);
		DCHK(hipGetLastError());
		lap(us_cls);
	}
	DCHK(hipMemcpy(tallies, d_ctr + 1, 16, hipMemcpyDeviceToHost));
	// the tally (1961-1986) runs while neither value is set; the thresholds (1989) are the partition's
	if (*max_chain == 0 && *max_sh == 0) { *max_chain = tallies[0]; *max_sh = tallies[1]; }
	if (*max_chain == 0 && tallies[0]) return fail(BHIP_E_ARG, "a later partition holds duplicate windows but the first tallied partition had none "
	                                                "(the reference divides by zero here); use fewer partitions (-dp)");
	const uint64_t sh1 = (uint64_t)(sqrt((double)*max_sh) / 2), sh2 = sh1 * 4 / 3, sh3 = sh1 * 3;
	DRES(d_flags, sym_len + 8);
	hipLaunchKernelGGL(k_dna_mark, dim3(grid_for(sym_len, 256, 65535)), dim3(256), 0, 0, d_cls.as<uint64_t>(), sym_len, sh1, sh2, sh3, *max_chain, d_flags.as<uint8_t>());
	DCHK(hipGetLastError());
	DCHK(hipMemcpy(flags, d_flags.p, sym_len, hipMemcpyDeviceToHost));
	lap(us_mark);
	if (dbg) fprintf(stderr, "[bhip] dna marks: %llu symbols, %llu eligible, %zu chunks (%llu exact), peak %.2f GB; upload %.1f ms, sort %.1f ms, classify %.1f ms, mark %.1f ms\n",
	                 (unsigned long long)sym_len, (unsigned long long)eligible, chunks.size(), (unsigned long long)exact_chunks, peak / 1e9, us_up / 1e3, us_sort / 1e3, us_cls / 1e3, us_mark / 1e3);
	if (info) {
		info[0] = eligible; info[1] = chunks.size(); info[2] = exact_chunks; info[3] = peak;
		info[4] = (uint64_t)us_up; info[5] = (uint64_t)us_sort; info[6] = (uint64_t)us_cls; info[7] = (uint64_t)us_mark;
	}
	return BHIP_OK;
}
