/* bh_paths.c -- alignment paths of the printed lines (burst_hip --cigar): the collector of what the report prints, the call that traces it
 * and the renderer of the two columns a line gets -- the leftmost 1-based position of the path on the ORIGINAL reference and the CIGAR
 * text in =XID.  No reference counterpart (the reference leaves "parse the alignments downstream" to its user); the path is defined in
 * include/burst_hip.h (bhip_trace_paths) and DESIGN.md section 3.
 *
 * The report renders chunks of unique queries into text as it always did (bh_report.c) and notes, per printed line, which record the
 * line shows and the offset of its reference (refStart).  A group of rendered chunks then comes here: the distinct records of the group
 * are traced in ONE call -- a record is one (query entry, refIx), so a duplicate read, or a lane that stands for several original
 * references, is traced once however many lines it has --, and every line is written again with its two columns behind everything it
 * had.  What stands in front of them is the bytes the run without the flag writes. */
#include "burst_host.h"
#include <stdlib.h>
#include <string.h>

struct BhPaths {
	bh_paths_trace_fn trace; void *ctx;
	uint64_t nRequests, nOps, nLines, nCalls;
	uint64_t shownRequests, shownOps, shownUs;      /* what bh_paths_print_info has reported so far */
	/* buffers kept between groups */
	uint64_t *idx; uint64_t idxCap;
	BhipPathReq *req; uint32_t *first, *gapr; uint64_t *off; uint64_t reqCap;
	uint32_t *ops; uint64_t opsCap;
	char *text; size_t textCap;
	/* who else gets the traced groups (bh_paths_set_collector: an entry with fn, bh_paths_add_collector: one with fn_text), in the order
	 * they were added; plain = the lines are written without the two columns */
	struct { bh_paths_collect_fn fn; bh_paths_collect_text_fn fn_text; void *ctx; } col[BH_PATHS_MAX_COLLECTORS];
	int nCol, plain;
};

static int trace_device(void *ctx, const BhQueries *Q, const BhipPathReq *req, uint64_t n, uint32_t *ops, uint64_t ops_cap, uint64_t *op_off,
                        uint32_t *ref_first, uint32_t *gap_r) {
	if (Q->numEntries > 0xFFFFFFFFull) return bh_set_error(BH_E_INTERNAL, "paths: %lu query entries", (unsigned long)Q->numEntries);
	const int rc = bhip_trace_paths(ctx, Q->codes, Q->qoff, (uint32_t)Q->numEntries, req, n, ops, ops_cap, op_off, ref_first, gap_r);
	if (rc == BHIP_E_CAPACITY) return BH_E_CAPACITY;
	if (rc) return bh_set_error(rc == BHIP_E_ARG || rc == BHIP_E_RESCORE || rc == BHIP_E_INTERNAL ? BH_E_INTERNAL : BH_E_DEVICE, "%s", bhip_last_error());
	return BH_OK;
}

int bh_paths_open(void *hip_handle, BhPaths **out) {
	BhPaths *p = calloc(1, sizeof(*p));
	if (!p) return bh_set_error(BH_E_OOM, "OOM:paths");
	p->trace = trace_device; p->ctx = hip_handle;
	*out = p;
	return BH_OK;
}
void bh_paths_set_trace(BhPaths *p, bh_paths_trace_fn fn, void *ctx) { p->trace = fn; p->ctx = ctx; }
static void col_remove(BhPaths *p, int k) { for (--p->nCol; k < p->nCol; ++k) p->col[k] = p->col[k + 1]; }
void bh_paths_set_collector(BhPaths *p, bh_paths_collect_fn fn, void *ctx, int columns) {
	if (!p) return;
	p->plain = !columns;
	int k = 0;
	while (k < p->nCol && !p->col[k].fn) ++k;
	if (!fn) { if (k < p->nCol) col_remove(p, k); return; }
	if (k == p->nCol) { if (p->nCol == BH_PATHS_MAX_COLLECTORS) return; ++p->nCol; }      /* (one entry of this kind: the list cannot fill up through here alone) */
	p->col[k].fn = fn; p->col[k].fn_text = NULL; p->col[k].ctx = ctx;
}
int bh_paths_add_collector(BhPaths *p, bh_paths_collect_text_fn fn, void *ctx, int columns) {
	if (!p || !fn) return bh_set_error(BH_E_USAGE, "bh_paths_add_collector: no tracer / no collector");
	p->plain = !columns;
	int k = 0;
	while (k < p->nCol && p->col[k].fn_text != fn) ++k;
	if (!ctx) { if (k < p->nCol) col_remove(p, k); return BH_OK; }
	if (k == p->nCol) { if (p->nCol == BH_PATHS_MAX_COLLECTORS) return bh_set_error(BH_E_USAGE, "bh_paths_add_collector: %d collectors already", p->nCol); ++p->nCol; }
	p->col[k].fn = NULL; p->col[k].fn_text = fn; p->col[k].ctx = ctx;
	return BH_OK;
}
void bh_paths_totals(const BhPaths *p, uint64_t *requests, uint64_t *ops, uint64_t *lines) {
	if (requests) *requests = p->nRequests;
	if (ops) *ops = p->nOps;
	if (lines) *lines = p->nLines;
}
/* one line on standard output: requests, ops and device time since the last such line (hip_handle: the one the paths are traced on) */
void bh_paths_print_info(BhPaths *p, void *hip_handle) {
	uint64_t info[4] = {0, 0, 0, 0};
	if (hip_handle) (void)bhip_paths_info(hip_handle, info);
	printf("Paths: %lu requests, %lu ops for %lu lines so far, %.3f ms on the device\n", (unsigned long)(p->nRequests - p->shownRequests), (unsigned long)(p->nOps - p->shownOps),
	       (unsigned long)p->nLines, (double)(info[1] - p->shownUs) / 1000.0);
	p->shownRequests = p->nRequests; p->shownOps = p->nOps; p->shownUs = info[1];
}
void bh_paths_close(BhPaths *p) {
	if (!p) return;
	free(p->idx); free(p->req); free(p->first); free(p->gapr); free(p->off); free(p->ops); free(p->text);
	free(p);
}

int bh_paths_push(BhPathBuf *b, uint64_t hit, uint32_t ref_off) { return bh_paths_push_line(b, hit, ref_off, 0, 1); }
int bh_paths_push_line(BhPathBuf *b, uint64_t hit, uint32_t ref_off, uint32_t header, int uniq) {
	if (b->n == b->cap) {
		const uint64_t nc = b->cap ? b->cap * 2 : 1024;
		BhPathLine *np = realloc(b->l, nc * sizeof(*np));
		if (!np) return 0;
		b->l = np; b->cap = nc;
	}
	b->l[b->n].hit = hit; b->l[b->n].refOff = ref_off; b->l[b->n].header = header; b->l[b->n].uniq = uniq != 0; ++b->n;
	return 1;
}

/* CIGAR text of n ops (words length << 4 | code; I = 1, D = 2, '=' = 7, X = 8): the length written, or 0 when `cap` bytes (the
 * terminating NUL included; 12 per op always suffice) are too few or a word holds another code or a zero length */
size_t bh_cigar_text(const uint32_t *ops, uint64_t n, char *out, size_t cap) {
	size_t len = 0;
	for (uint64_t i = 0; i < n; ++i) {
		uint32_t v = ops[i] >> 4; const uint32_t code = ops[i] & 15u;
		const char c = code == BHIP_OP_EQ ? '=' : code == BHIP_OP_X ? 'X' : code == BHIP_OP_I ? 'I' : code == BHIP_OP_D ? 'D' : 0;
		if (!c || !v) return 0;
		char t[12]; int k = 0;
		do { t[k++] = (char)('0' + v % 10); v /= 10; } while (v);
		if (len + (size_t)k + 2 > cap) return 0;
		while (k) out[len++] = t[--k];
		out[len++] = c;
	}
	if (len + 1 > cap) return 0;
	out[len] = 0;
	return len;
}

static int cmp_u64(const void *a, const void *b) { const uint64_t x = *(const uint64_t *)a, y = *(const uint64_t *)b; return x < y ? -1 : x > y; }

#define GROW(ptr, capvar, need, type) do { if ((need) > (capvar)) { uint64_t nc_ = (capvar) ? (capvar) * 2 : 1024; while (nc_ < (need)) nc_ *= 2; \
	type *np_ = realloc(ptr, nc_ * sizeof(type)); if (!np_) return bh_set_error(BH_E_OOM, "OOM:paths"); ptr = np_; capvar = nc_; } } while (0)

int bh_paths_emit(BhPaths *p, FILE *out, const BhQueries *Q, const BhipHit *hits, char *const *text, const size_t *text_len, const BhPathBuf *bufs, uint64_t n_chunks) {
	uint64_t nl = 0;
	for (uint64_t c = 0; c < n_chunks; ++c) nl += bufs[c].n;
	if (!nl) {
		for (uint64_t c = 0; c < n_chunks; ++c) if (text_len[c]) return bh_set_error(BH_E_INTERNAL, "paths: %lu bytes of text without a line record", (unsigned long)text_len[c]);
		return BH_OK;
	}
	/* the distinct records of the group, ascending */
	GROW(p->idx, p->idxCap, nl, uint64_t);
	uint64_t k = 0;
	for (uint64_t c = 0; c < n_chunks; ++c) for (uint64_t i = 0; i < bufs[c].n; ++i) p->idx[k++] = bufs[c].l[i].hit;
	qsort(p->idx, nl, sizeof(*p->idx), cmp_u64);
	uint64_t nr = 0;
	for (uint64_t i = 0; i < nl; ++i) if (!nr || p->idx[nr - 1] != p->idx[i]) p->idx[nr++] = p->idx[i];
	if (nr + 1 > p->reqCap) {
		uint64_t nc = p->reqCap ? p->reqCap : 1024;
		while (nc < nr + 1) nc *= 2;
		BhipPathReq *a = realloc(p->req, nc * sizeof(*a)); if (a) p->req = a;
		uint32_t *b = realloc(p->first, nc * sizeof(*b)); if (b) p->first = b;
		uint32_t *g = realloc(p->gapr, nc * sizeof(*g)); if (g) p->gapr = g;
		uint64_t *o = realloc(p->off, nc * sizeof(*o)); if (o) p->off = o;
		if (!a || !b || !g || !o) return bh_set_error(BH_E_OOM, "OOM:paths");
		p->reqCap = nc;
	}
	for (uint64_t i = 0; i < nr; ++i) {
		const BhipHit *h = hits + p->idx[i];
		p->req[i].q = h->q; p->req[i].refIx = h->refIx; p->req[i].finalPos = h->finalPos; p->req[i].ed = h->ed;
	}
	GROW(p->ops, p->opsCap, 8 * nr, uint32_t);
	int rc = p->trace(p->ctx, Q, p->req, nr, p->ops, p->opsCap, p->off, p->first, p->gapr);
	if (rc == BH_E_CAPACITY) {
		GROW(p->ops, p->opsCap, p->off[nr], uint32_t);
		rc = p->trace(p->ctx, Q, p->req, nr, p->ops, p->opsCap, p->off, p->first, p->gapr);
		if (rc == BH_E_CAPACITY) return bh_set_error(BH_E_INTERNAL, "paths: %lu ops do not fit the room the first call asked for", (unsigned long)p->off[nr]);
	}
	if (rc) return rc;
	p->nRequests += nr; p->nOps += p->off[nr]; p->nLines += nl; ++p->nCalls;
	for (int k = 0; k < p->nCol; ++k) {
		rc = p->col[k].fn ? p->col[k].fn(p->col[k].ctx, p->idx, p->req, p->first, p->off, p->ops, nr, bufs, n_chunks)
		                  : p->col[k].fn_text(p->col[k].ctx, p->idx, p->req, p->first, p->off, p->ops, nr, bufs, text, text_len, n_chunks);
		if (rc) return rc;
	}
	if (p->plain) {      /* the lines as they were rendered */
		for (uint64_t c = 0; c < n_chunks; ++c) if (text_len[c] && fwrite(text[c], 1, text_len[c], out) != text_len[c]) return bh_set_error(BH_E_IO, "short write on the output file");
		return BH_OK;
	}
	/* every line again, its two columns behind what it had */
	for (uint64_t c = 0; c < n_chunks; ++c) {
		const char *s = text[c], *end = s + text_len[c];
		size_t len = 0;
		for (uint64_t i = 0; i < bufs[c].n; ++i) {
			const char *nlp = s < end ? memchr(s, '\n', (size_t)(end - s)) : NULL;
			if (!nlp) return bh_set_error(BH_E_INTERNAL, "paths: %lu line records, fewer lines of text", (unsigned long)bufs[c].n);
			const uint64_t key = bufs[c].l[i].hit;
			uint64_t lo = 0, hi = nr;      /* (the record is there: it was put there above) */
			while (lo + 1 < hi) { const uint64_t mid = (lo + hi) / 2; if (p->idx[mid] <= key) lo = mid; else hi = mid; }
			const uint64_t n_ops = p->off[lo + 1] - p->off[lo];
			const size_t need = (size_t)(nlp - s) + 16 + 12 * n_ops + 4;
			if (len + need > p->textCap) {
				size_t nc = p->textCap ? p->textCap * 2 : (1u << 20);
				while (nc < len + need) nc *= 2;
				char *np = realloc(p->text, nc);
				if (!np) return bh_set_error(BH_E_OOM, "OOM:paths");
				p->text = np; p->textCap = nc;
			}
			memcpy(p->text + len, s, (size_t)(nlp - s)); len += (size_t)(nlp - s);
			p->text[len++] = '\t';
			{ uint64_t v = (uint64_t)bufs[c].l[i].refOff + p->first[lo]; char t[24]; int d = 0; do { t[d++] = (char)('0' + v % 10); v /= 10; } while (v); while (d) p->text[len++] = t[--d]; }
			p->text[len++] = '\t';
			const size_t cl = bh_cigar_text(p->ops + p->off[lo], n_ops, p->text + len, 12 * n_ops + 2);
			if (!cl) return bh_set_error(BH_E_INTERNAL, "paths: record %lu has a path of %lu ops that does not render", (unsigned long)key, (unsigned long)n_ops);
			len += cl;
			p->text[len++] = '\n';
			s = nlp + 1;
		}
		if (s != end) return bh_set_error(BH_E_INTERNAL, "paths: more lines of text than line records");
		if (len && fwrite(p->text, 1, len, out) != len) return bh_set_error(BH_E_IO, "short write on the output file");
	}
	return BH_OK;
}
