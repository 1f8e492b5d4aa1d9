/* bh_mates.c -- paired-end reads (burst_hip --mates): the collector of two mates' printed placements, the call that joins them and the
 * writer of the paired output.  No reference counterpart: the reference lists "paired-end unstitched alignments" as planned and names
 * the recipe (both mates in ALLPATHS mode, then the references both map to with acceptable orientation and distance); the definition is in
 * the README ("Paired-end reads") and include/burst_hip.h (bhip_mates_join).
 *
 * Everything is a function of the LINES the two single-end runs print, so that is what the collector takes: the session (bh_session.c)
 * sends each mate through its ordinary per-sample path into a temporary file beside the output, and bh_mates_join_files reads the two
 * texts back.  A line gives its read (column 1), header (column 2), st / ed (columns 9 and 10, signed 32-bit) and edits (column 11); pair
 * names (column 1 without a trailing /1 or /2) and headers are numbered densely by one string table, the join runs on those numbers
 * (bhip_mates_join on the reporting rank's handle, or the function bh_mates_set_join put in its place), and every reported combination is
 * written as its two lines, each followed by the fragment's leftmost position and length.
 *
 * Buffering: spilled.  Mate 1's text waits in its temporary file while mate 2 is searched; during the join both texts are in memory once
 * (their bytes + 28 bytes per line + the read names of both files), nothing else grows with the input, and the temporary files are removed
 * whatever the outcome. */
#include "burst_host.h"
#include <stdlib.h>
#include <string.h>

/* strings -> dense numbers: open addressing over copies kept in one arena */
typedef struct StrTab { char *arena; size_t used, cap; uint64_t *off; uint32_t *len; uint32_t n, ncap; uint32_t *slot; uint64_t nslot; } StrTab;
static uint64_t str_hash(const char *s, size_t n) { uint64_t h = 1469598103934665603ull; for (size_t i = 0; i < n; ++i) { h ^= (uint8_t)s[i]; h *= 1099511628211ull; } return h ^ (h >> 29); }
static void strtab_free(StrTab *t) { free(t->arena); free(t->off); free(t->len); free(t->slot); memset(t, 0, sizeof *t); }
static int strtab_rehash(StrTab *t, uint64_t nslot) {
	uint32_t *s = malloc(nslot * sizeof(*s));
	if (!s) return 0;
	memset(s, 0xFF, nslot * sizeof(*s));
	for (uint32_t i = 0; i < t->n; ++i) { uint64_t p = str_hash(t->arena + t->off[i], t->len[i]) & (nslot - 1); while (s[p] != 0xFFFFFFFFu) p = (p + 1) & (nslot - 1); s[p] = i; }
	free(t->slot); t->slot = s; t->nslot = nslot;
	return 1;
}
/* number of the string, added when `add`; 0xFFFFFFFF = not there (add = 0) or no memory (add = 1) */
static uint32_t strtab_get(StrTab *t, const char *s, size_t n, int add) {
	if (!t->nslot) { if (!add) return 0xFFFFFFFFu; if (!strtab_rehash(t, 1024)) return 0xFFFFFFFFu; }
	uint64_t p = str_hash(s, n) & (t->nslot - 1);
	for (; t->slot[p] != 0xFFFFFFFFu; p = (p + 1) & (t->nslot - 1)) { const uint32_t i = t->slot[p]; if (t->len[i] == n && !memcmp(t->arena + t->off[i], s, n)) return i; }
	if (!add || t->n == 0xFFFFFFFEu) return 0xFFFFFFFFu;
	if (((uint64_t)t->n + 1) * 2 > t->nslot) {      /* grown BEFORE the string goes in: a failure leaves the table as it was */
		if (!strtab_rehash(t, t->nslot * 2)) return 0xFFFFFFFFu;
		for (p = str_hash(s, n) & (t->nslot - 1); t->slot[p] != 0xFFFFFFFFu; p = (p + 1) & (t->nslot - 1)) { }
	}
	if (t->n == t->ncap) {
		const uint32_t nc = t->ncap ? (t->ncap < 0x7FFFFFFFu ? t->ncap * 2 : 0xFFFFFFFEu) : 1024;
		uint64_t *no = realloc(t->off, (size_t)nc * sizeof(*no)); if (!no) return 0xFFFFFFFFu; t->off = no;
		uint32_t *nl = realloc(t->len, (size_t)nc * sizeof(*nl)); if (!nl) return 0xFFFFFFFFu; t->len = nl;
		t->ncap = nc;
	}
	if (t->used + n > t->cap) { const size_t nc = (t->cap ? t->cap * 2 : 1 << 16) + n; char *na = realloc(t->arena, nc); if (!na) return 0xFFFFFFFFu; t->arena = na; t->cap = nc; }
	memcpy(t->arena + t->used, s, n);
	const uint32_t id = t->n++;
	t->off[id] = t->used; t->len[id] = (uint32_t)n; t->used += n;
	t->slot[p] = id;
	return id;
}

struct BhMates {
	bh_mates_join_fn join; void *ctx; void *hh;
	StrTab pairs;                    /* pair names of the two files' reads, then of whatever else the texts name */
	uint8_t *flag; uint32_t flagCap; /* per pair: 1 named in file 1, 2 named in file 2, 4 / 8 placed by mate 1 / 2 */
	BhMatesStats st;
	uint64_t shownUs;
};

static int join_device(void *ctx, const BhipMateLine *a, uint64_t na, const BhipMateLine *b, uint64_t nb, uint32_t orientation, uint32_t ins_min, uint32_t ins_max,
                       uint32_t report, uint32_t *out_a, uint32_t *out_b, uint64_t cap, uint64_t *n_out) {
	BhMates *m = ctx;
	if (!m->hh) return bh_set_error(BH_E_USAGE, "mates: no device handle on the reporting rank and no joiner in its place");
	const int rc = bhip_mates_join(m->hh, a, na, b, nb, orientation, ins_min, ins_max, report, out_a, out_b, cap, n_out);
	if (rc == BHIP_E_CAPACITY) return BH_E_CAPACITY;
	if (rc) return bh_set_error(rc == BHIP_E_ARG || rc == BHIP_E_INTERNAL ? BH_E_INTERNAL : BH_E_DEVICE, "%s", bhip_last_error());
	return BH_OK;
}

int bh_mates_open(void *hip_handle, BhMates **out) {
	BhMates *m = calloc(1, sizeof(*m));
	if (!m) return bh_set_error(BH_E_OOM, "OOM:mates");
	m->join = join_device; m->ctx = m; m->hh = hip_handle;
	*out = m;
	return BH_OK;
}
void bh_mates_set_handle(BhMates *m, void *hip_handle) { m->hh = hip_handle; }
void bh_mates_set_join(BhMates *m, bh_mates_join_fn fn, void *ctx) { if (fn) { m->join = fn; m->ctx = ctx; } else { m->join = join_device; m->ctx = m; } }
void bh_mates_stats(const BhMates *m, BhMatesStats *st) { *st = m->st; }
void bh_mates_close(BhMates *m) {
	if (!m) return;
	strtab_free(&m->pairs); free(m->flag);
	free(m);
}
void bh_mates_print_info(const BhMates *m) {
	const BhMatesStats *s = &m->st;
	printf("Mates: %lu + %lu reads, %lu pairs named in both files, %lu placed on both sides; %lu + %lu lines, %lu combinations examined, %lu written; %.3f ms on the device\n",
	       (unsigned long)s->reads1, (unsigned long)s->reads2, (unsigned long)s->pairsNamed, (unsigned long)s->pairsPlaced, (unsigned long)s->lines1, (unsigned long)s->lines2,
	       (unsigned long)s->examined, (unsigned long)s->written, s->deviceMs);
}

static size_t pair_name_len(const char *s, size_t n) { return n >= 2 && s[n - 2] == '/' && (s[n - 1] == '1' || s[n - 1] == '2') ? n - 2 : n; }
static uint32_t pair_of(BhMates *m, const char *s, size_t n, uint8_t bit) {
	const uint32_t id = strtab_get(&m->pairs, s, pair_name_len(s, n), 1);
	if (id == 0xFFFFFFFFu) return id;
	if (id >= m->flagCap) {
		const uint32_t nc = id < 0x7FFFFFFFu ? (id + 1024) * 2 : 0xFFFFFFFFu;
		uint8_t *nf = realloc(m->flag, nc); if (!nf) return 0xFFFFFFFFu;
		memset(nf + m->flagCap, 0, nc - m->flagCap); m->flag = nf; m->flagCap = nc;
	}
	m->flag[id] |= bit;
	return id;
}

/* a new pair of files: side 0 first.  heads = the read names of the file as column 1 prints them */
int bh_mates_names(BhMates *m, int side, char *const *heads, uint64_t n) {
	if (!side) { strtab_free(&m->pairs); free(m->flag); m->flag = NULL; m->flagCap = 0; memset(&m->st, 0, sizeof m->st); }
	for (uint64_t i = 0; i < n; ++i) if (pair_of(m, heads[i], strlen(heads[i]), side ? 2 : 1) == 0xFFFFFFFFu) return bh_set_error(BH_E_OOM, "OOM:mates (read names)");
	if (side) m->st.reads2 = n; else m->st.reads1 = n;
	return BH_OK;
}

typedef struct MText { char *text; size_t size; uint64_t *off; BhipMateLine *l; uint64_t n; } MText;
static void mtext_free(MText *t) { free(t->text); free(t->off); free(t->l); memset(t, 0, sizeof *t); }
static int mtext_read(MText *t, const char *path) {
	FILE *f = fopen(path, "rb");
	if (!f) return bh_set_error(BH_E_IO, "ERROR: Cannot open the mate's lines: %s", path);
	int ok = !fseek(f, 0, SEEK_END);
	const long sz = ok ? ftell(f) : -1;
	ok = ok && sz >= 0 && !fseek(f, 0, SEEK_SET);
	if (ok && !(t->text = malloc((size_t)sz + 1))) { fclose(f); return bh_set_error(BH_E_OOM, "OOM:mates (%ld bytes of lines)", sz); }
	ok = ok && fread(t->text, 1, (size_t)sz, f) == (size_t)sz;
	fclose(f);
	if (!ok) return bh_set_error(BH_E_IO, "ERROR: Cannot read the mate's lines: %s", path);
	t->size = (size_t)sz; t->text[sz] = 0;
	return BH_OK;
}
/* the lines of a text: offsets (n + 1) and the five fields of each; pair and header numbers from the two tables */
static int mtext_parse(MText *t, BhMates *m, StrTab *refs, uint8_t placed_bit) {
	uint64_t n = 0;
	for (size_t i = 0; i < t->size; ++i) n += t->text[i] == '\n';
	if (t->size && t->text[t->size - 1] != '\n') ++n;
	if (n >= 0xFFFFFFFFull) return bh_set_error(BH_E_USAGE, "mates: %lu lines of one mate (fewer than 2^32)", (unsigned long)n);
	t->off = malloc((n + 1) * sizeof(*t->off)); t->l = malloc((n ? n : 1) * sizeof(*t->l));
	if (!t->off || !t->l) return bh_set_error(BH_E_OOM, "OOM:mates (%lu lines)", (unsigned long)n);
	size_t p = 0;
	for (uint64_t k = 0; k < n; ++k) {
		const char *s = t->text + p, *e = memchr(s, '\n', t->size - p);
		if (!e) e = t->text + t->size;
		t->off[k] = p;
		const char *col[12]; int nc = 0;
		col[nc++] = s;
		for (const char *q = s; q < e && nc < 12; ++q) if (*q == '\t') col[nc++] = q + 1;
		if (nc < 12) return bh_set_error(BH_E_INTERNAL, "mates: line %lu of a mate's output has %d columns", (unsigned long)k + 1, nc);
		BhipMateLine *l = &t->l[k];
		l->pair = pair_of(m, col[0], (size_t)(col[1] - 1 - col[0]), placed_bit);
		l->ref = strtab_get(refs, col[1], (size_t)(col[2] - 1 - col[1]), 1);
		if (l->pair == 0xFFFFFFFFu || l->ref == 0xFFFFFFFFu) return bh_set_error(BH_E_OOM, "OOM:mates (names)");
		l->st = (int32_t)(uint32_t)strtoll(col[8], NULL, 10); l->ed = (int32_t)(uint32_t)strtoll(col[9], NULL, 10);
		l->edits = (uint32_t)strtoul(col[10], NULL, 10);
		p = (size_t)(e - t->text) + (e < t->text + t->size);
	}
	t->off[n] = p; t->n = n;
	return BH_OK;
}

/* The pair numbers of the lines, made dense over the pairs that HAVE lines.  The names table numbers every read of both files (the
 * statistics need them), and of a shotgun sample a minority places: numbers that follow the reads would leave the joiner a table of
 * mostly unused pairs, and bhip_mates_join refuses `best` for numbers that are not dense relative to the lines. */
static int renumber_pairs(MText *A, MText *B, uint32_t n_names, uint32_t *n_pairs) {
	uint32_t *map = malloc(((size_t)n_names + 1) * sizeof(*map));
	if (!map) return bh_set_error(BH_E_OOM, "OOM:mates (pair numbers)");
	memset(map, 0xFF, ((size_t)n_names + 1) * sizeof(*map));
	uint32_t next = 0;
	MText *T[2] = {A, B};
	for (int k = 0; k < 2; ++k) for (uint64_t i = 0; i < T[k]->n; ++i) {
		uint32_t *q = &map[T[k]->l[i].pair];
		if (*q == 0xFFFFFFFFu) *q = next++;
		T[k]->l[i].pair = *q;
	}
	free(map);
	*n_pairs = next;
	return BH_OK;
}

/* pairs of lines with equal (pair, header): what the join looks at */
static int count_examined(const MText *A, const MText *B, uint64_t *out) {
	uint64_t nslot = 1024;
	while (nslot < 2 * B->n + 2) nslot *= 2;
	uint64_t *key = malloc(nslot * sizeof(*key)); uint32_t *cnt = calloc(nslot, sizeof(*cnt));
	if (!key || !cnt) { free(key); free(cnt); return bh_set_error(BH_E_OOM, "OOM:mates"); }
	memset(key, 0xFF, nslot * sizeof(*key));      /* (no line has pair and header 0xFFFFFFFF: the tables hold fewer strings) */
	for (uint64_t i = 0; i < B->n; ++i) {
		const uint64_t k = (uint64_t)B->l[i].pair << 32 | B->l[i].ref;
		uint64_t p = (k * 0x9E3779B97F4A7C15ull) >> 20 & (nslot - 1);
		while (key[p] != ~0ull && key[p] != k) p = (p + 1) & (nslot - 1);
		key[p] = k; ++cnt[p];
	}
	uint64_t tot = 0;
	for (uint64_t i = 0; i < A->n; ++i) {
		const uint64_t k = (uint64_t)A->l[i].pair << 32 | A->l[i].ref;
		uint64_t p = (k * 0x9E3779B97F4A7C15ull) >> 20 & (nslot - 1);
		while (key[p] != ~0ull && key[p] != k) p = (p + 1) & (nslot - 1);
		if (key[p] == k) tot += cnt[p];
	}
	free(key); free(cnt);
	*out = tot;
	return BH_OK;
}

/* leftmost position and length of a reported combination (the upstream line's lo, the downstream line's hi: bhip_mates_join) */
static void fragment_of(const BhipMateLine *a, const BhipMateLine *b, uint32_t orientation, long long *left, long long *len) {
	const int ra = a->st > a->ed;
	const int a_up = orientation == BHIP_MATES_FF ? !ra : orientation == BHIP_MATES_FR ? !ra : ra;
	const BhipMateLine *U = a_up ? a : b, *D = a_up ? b : a;
	const long long ulo = U->st < U->ed ? U->st : U->ed, dhi = D->st < D->ed ? D->ed : D->st;
	*left = ulo; *len = dhi - ulo + 1;
}

int bh_mates_join_files(BhMates *m, const char *lines1, const char *lines2, FILE *out, const BhMatesOpts *o, uint64_t *n_lines) {
	MText A, B; StrTab refs;
	memset(&A, 0, sizeof A); memset(&B, 0, sizeof B); memset(&refs, 0, sizeof refs);
	uint32_t *oa = NULL, *ob = NULL;
	uint64_t n = 0, cap = 0;
	int rc = mtext_read(&A, lines1);
	if (!rc) rc = mtext_read(&B, lines2);
	if (!rc) rc = mtext_parse(&A, m, &refs, 4);
	if (!rc) rc = mtext_parse(&B, m, &refs, 8);
	uint32_t n_line_pairs = 0;
	if (!rc) rc = renumber_pairs(&A, &B, m->pairs.n, &n_line_pairs);
	if (!rc) rc = count_examined(&A, &B, &m->st.examined);
	if (!rc) {
		m->st.lines1 = A.n; m->st.lines2 = B.n;
		for (uint32_t i = 0; i < m->pairs.n && i < m->flagCap; ++i) { m->st.pairsNamed += (m->flag[i] & 3) == 3; m->st.pairsPlaced += m->flag[i] == 15; }
		/* room for every combination examined: an upper bound of what any report returns, so the device joiner never answers with a
		 * capacity; another joiner's capacity answer names the room it wants and is tried once more */
		cap = m->st.examined ? m->st.examined : 1;
		for (int attempt = 0; attempt < 2; ++attempt) {
			free(oa); free(ob);
			oa = malloc(cap * sizeof(*oa)); ob = malloc(cap * sizeof(*ob));
			if (!oa || !ob) { rc = bh_set_error(BH_E_OOM, "OOM:mates (%lu combinations)", (unsigned long)cap); break; }
			n = 0;
			rc = m->join(m->ctx, A.l, A.n, B.l, B.n, o->orientation, o->ins_min, o->ins_max, o->report, oa, ob, cap, &n);
			if (rc != BH_E_CAPACITY) break;
			if (attempt || n <= cap) { rc = bh_set_error(BH_E_INTERNAL, "mates: the joiner wants room for %lu combinations after being given %lu", (unsigned long)n, (unsigned long)cap); break; }
			cap = n;
		}
	}
	if (!rc && n > cap) rc = bh_set_error(BH_E_INTERNAL, "mates: the joiner returned %lu combinations in room for %lu", (unsigned long)n, (unsigned long)cap);
	for (uint64_t i = 0; !rc && i < n; ++i) {
		if (oa[i] >= A.n || ob[i] >= B.n) { rc = bh_set_error(BH_E_INTERNAL, "mates: combination %lu names lines %u and %u of %lu and %lu", (unsigned long)i, oa[i], ob[i], (unsigned long)A.n, (unsigned long)B.n); break; }
		long long left, len; char tail[64];
		fragment_of(&A.l[oa[i]], &B.l[ob[i]], o->orientation, &left, &len);
		const int tl = snprintf(tail, sizeof tail, "\t%lld\t%lld\n", left, len);
		const char *sa = A.text + A.off[oa[i]], *sb = B.text + B.off[ob[i]];
		size_t la = (size_t)(A.off[oa[i] + 1] - A.off[oa[i]]), lb = (size_t)(B.off[ob[i] + 1] - B.off[ob[i]]);
		if (la && sa[la - 1] == '\n') --la;
		if (lb && sb[lb - 1] == '\n') --lb;
		if (fwrite(sa, 1, la, out) != la || fwrite(tail, 1, (size_t)tl, out) != (size_t)tl || fwrite(sb, 1, lb, out) != lb || fwrite(tail, 1, (size_t)tl, out) != (size_t)tl)
			rc = bh_set_error(BH_E_IO, "ERROR: write failed (paired output)");
	}
	if (!rc) {
		m->st.written = n;
		if (n_lines) *n_lines = 2 * n;
		if (m->join == join_device && m->hh) { uint64_t info[4] = {0, 0, 0, 0}; (void)bhip_mates_info(m->hh, info); m->st.deviceMs = (double)(info[1] - m->shownUs) / 1000.0; m->shownUs = info[1]; }
	}
	free(oa); free(ob); mtext_free(&A); mtext_free(&B); strtab_free(&refs);
	return rc;
}
