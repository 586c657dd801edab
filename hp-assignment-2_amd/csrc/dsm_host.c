/*
 * dsm_host.c -- host side of the drop-in boundary (part of libdsm.so; no GPU involved).
 *
 *   dsm_parse_trace_file / dsm_load_test_dir  replace initializeProcessor's trace reader
 *                                             (assignment.c:792-818)
 *   dsm_format_dump / dsm_write_dump          replace printProcessorState (:824-876),
 *                                             byte-for-byte
 *   dsm_parse_dump / dsm_read_dump            their inverse: an output file back into a record
 *   dsm_node_hash                             canonical 64-bit hash of a node record
 *   dsm_outcome_key / dsm_census_results / _insert / _merge / _sorted / _find
 *                                             the outcome census on the host
 *   dsm_audit_states / _merge / _class_name   the coherence audit on the host
 */
#include "dsm.h"

#include <errno.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

const char *dsm_strerror(int code) {
    switch (code) {
    case DSM_OK: return "ok";
    case DSM_E_INVAL: return "invalid argument";
    case DSM_E_DEVICE: return "no usable gfx950 device or HIP runtime error";
    case DSM_E_NOMEM: return "out of memory";
    case DSM_E_IO: return "file could not be opened or written";
    case DSM_E_FORMAT: return "trace line is neither 'RD <addr>' nor 'WR <addr> <value>'";
    case DSM_E_STATE: return "operation not valid in the current context state";
    case DSM_E_RANGE: return "address outside the simulated nodes (home >= np)";
    default: return "unknown error";
    }
}

int dsm_abi_version(void) { return DSM_ABI_VERSION; }

/* Same chunking as :802-818: fgets into a 20-byte buffer, the count is checked after the
 * read (so line cap+1 is consumed and dropped), %hhx / %hhu store modulo 256. */
int dsm_parse_trace_file(const char *path, uint16_t *out, uint32_t cap, uint32_t *count) {
    if (!path || !count || (cap && !out)) return DSM_E_INVAL;
    FILE *f = fopen(path, "r");
    if (!f) return DSM_E_IO;
    char line[20];
    uint32_t n = 0;
    int rc = DSM_OK;
    while (fgets(line, sizeof line, f) && n < cap) {
        unsigned char a = 0, v = 0;
        int wr;
        if (line[0] == 'R' && line[1] == 'D') {
            if (sscanf(line, "RD %hhx", &a) != 1) { rc = DSM_E_FORMAT; break; }
            wr = 0; v = 0;                                   /* :807-810 */
        } else if (line[0] == 'W' && line[1] == 'R') {
            if (sscanf(line, "WR %hhx %hhu", &a, &v) != 2) { rc = DSM_E_FORMAT; break; }
            wr = 1;                                          /* :811-815 */
        } else {
            rc = DSM_E_FORMAT;  /* the reference counts this chunk with garbage contents */
            break;
        }
        if (a > 0x7F) { rc = DSM_E_RANGE; break; }
        out[n++] = (uint16_t)((wr << 15) | (a << 8) | v);
    }
    fclose(f);
    *count = n;
    return rc;
}

int dsm_load_test_dir(const char *dir_name, int np, uint32_t cap, uint16_t *traces,
                      uint32_t stride, uint32_t *counts) {
    if (!dir_name || !traces || !counts || (np != 4 && np != 8) || cap > stride)
        return DSM_E_INVAL;
    for (int n = 0; n < np; ++n) {
        char path[256];
        snprintf(path, sizeof path, "tests/%s/core_%d.txt", dir_name, n);   /* :794 */
        int rc = dsm_parse_trace_file(path, traces + (size_t)n * stride, cap, &counts[n]);
        if (rc) return rc;
        for (uint32_t i = 0; i < counts[n]; ++i)
            if (((traces[(size_t)n * stride + i] >> 12) & 0x7) >= (unsigned)np)
                return DSM_E_RANGE;
    }
    return DSM_OK;
}

int dsm_format_dump(int node, const dsm_node_state *st, char *buf, size_t cap) {
    static const char *cst[] = {"MODIFIED", "EXCLUSIVE", "SHARED", "INVALID"};  /* :826 */
    static const char *dst[] = {"EM", "S", "U"};                                /* :828 */
    if (!st || !buf) return DSM_E_INVAL;
    size_t n = 0;
#define EMIT(...)                                                                    \
    do {                                                                             \
        int k_ = snprintf(buf + n, cap - n, __VA_ARGS__);                            \
        if (k_ < 0 || (size_t)k_ >= cap - n) return DSM_E_INVAL;                     \
        n += (size_t)k_;                                                             \
    } while (0)
    EMIT("=======================================\n");
    EMIT(" Processor Node: %d\n", node);
    EMIT("=======================================\n\n");
    EMIT("-------- Memory State --------\n");
    EMIT("| Index | Address |   Value  |\n");
    EMIT("|----------------------------|\n");
    for (int i = 0; i < DSM_MEM_SIZE; i++)
        EMIT("|  %3d  |  0x%02X   |  %5d   |\n", i, (node << 4) + i, st->memory[i]);
    EMIT("------------------------------\n\n");
    EMIT("------------ Directory State ---------------\n");
    EMIT("| Index | Address | State |    BitVector   |\n");
    EMIT("|------------------------------------------|\n");
    for (int i = 0; i < DSM_MEM_SIZE; i++)
        EMIT("|  %3d  |  0x%02X   |  %2s   |   0x%08X   |\n", i, (node << 4) + i,
             st->dir_state[i] < 3 ? dst[st->dir_state[i]] : "??", st->dir_bv[i]);
    EMIT("--------------------------------------------\n\n");
    EMIT("------------ Cache State ----------------\n");
    EMIT("| Index | Address | Value |    State    |\n");
    EMIT("|---------------------------------------|\n");
    for (int i = 0; i < DSM_CACHE_SIZE; i++)
        EMIT("|  %3d  |  0x%02X   |  %3d  |  %8s \t|\n", i, st->cache_addr[i],
             st->cache_value[i], st->cache_state[i] < 4 ? cst[st->cache_state[i]] : "????");
    EMIT("----------------------------------------\n\n");
#undef EMIT
    return (int)n;
}

int dsm_write_dump(int node, const dsm_node_state *st, const char *dir) {
    char buf[4096], path[512];
    int len = dsm_format_dump(node, st, buf, sizeof buf);
    if (len < 0) return len;
    if (dir) snprintf(path, sizeof path, "%s/core_%d_output.txt", dir, node);
    else snprintf(path, sizeof path, "core_%d_output.txt", node);         /* :831 */
    FILE *f = fopen(path, "w");
    if (!f) return DSM_E_IO;
    size_t w = fwrite(buf, 1, (size_t)len, f);
    int rc = fclose(f);
    return (w == (size_t)len && rc == 0) ? DSM_OK : DSM_E_IO;
}

/* ---- the dump reader (include/dsm.h): the plain reference of unfmt_kernel (dsm_text.hip) ----
 * Acceptance is the formatter's: the 55 lines are scanned loosely with sscanf, the record that
 * scan yields is formatted again, and only a text equal to that byte for byte is accepted. */

/* index of `s` among names[0 .. n), or -1 */
static int name_index(const char *s, const char *const *names, int n) {
    for (int i = 0; i < n; ++i)
        if (!strcmp(s, names[i])) return i;
    return -1;
}

/* z is cut into its lines in place (sscanf measures its whole input on every call) */
static int parse_dump_loose(char *z, int *node, dsm_node_state *st) {
    static const char *const cst[] = {"MODIFIED", "EXCLUSIVE", "SHARED", "INVALID"};
    static const char *const dst[] = {"EM", "S", "U"};
    const char *line[55];
    int nl = 0;
    for (char *p = z; *p && nl < 55; ++nl) {            /* line starts */
        line[nl] = p;
        char *e = strchr(p, '\n');
        if (!e) return DSM_E_FORMAT;
        *e = 0;
        p = e + 1;
    }
    if (nl != 55) return DSM_E_FORMAT;
    int idx, nd;
    unsigned a, b;
    char s[16];
    if (sscanf(line[1], " Processor Node: %9d", &nd) != 1 || nd < 0 || nd >= DSM_MAX_NP) return DSM_E_FORMAT;
    for (int i = 0; i < DSM_MEM_SIZE; ++i) {            /* lines 7 .. 22 */
        int v;
        if (sscanf(line[7 + i], "| %9d | %8x | %9d |", &idx, &a, &v) != 3) return DSM_E_FORMAT;
        st->memory[i] = (uint8_t)v;
    }
    for (int i = 0; i < DSM_MEM_SIZE; ++i) {            /* lines 28 .. 43 */
        if (sscanf(line[28 + i], "| %9d | %8x | %2s | %10x |", &idx, &a, s, &b) != 4) return DSM_E_FORMAT;
        const int d = name_index(s, dst, 3);
        if (d < 0) return DSM_E_FORMAT;
        st->dir_state[i] = (uint8_t)d;
        st->dir_bv[i] = (uint8_t)b;
    }
    for (int i = 0; i < DSM_CACHE_SIZE; ++i) {          /* lines 49 .. 52 */
        int v;
        if (sscanf(line[49 + i], "| %9d | %8x | %9d | %9s", &idx, &a, &v, s) != 4) return DSM_E_FORMAT;
        const int c = name_index(s, cst, 4);
        if (c < 0) return DSM_E_FORMAT;
        st->cache_addr[i] = (uint8_t)a;
        st->cache_value[i] = (uint8_t)v;
        st->cache_state[i] = (uint8_t)c;
    }
    *node = nd;
    return DSM_OK;
}

int dsm_parse_dump(const char *text, size_t len, int *node, dsm_node_state *st) {
    if (!node || !st || (len && !text)) return DSM_E_INVAL;
    char z[DSM_DUMP_MAX + 1], again[DSM_DUMP_MAX + 2];
    dsm_node_state r;
    int nd = -1;
    memset(&r, 0, sizeof r);
    int rc = DSM_E_FORMAT;
    if (len >= DSM_DUMP_BASE && len <= DSM_DUMP_MAX) {
        memcpy(z, text, len);
        z[len] = 0;
        r.flags = 0x02;
        if (strlen(z) == len && parse_dump_loose(z, &nd, &r) == DSM_OK &&
            dsm_format_dump(nd, &r, again, sizeof again) == (int)len && !memcmp(again, text, len))
            rc = DSM_OK;
    }
    if (rc != DSM_OK) {
        nd = -1;
        memset(&r, 0, sizeof r);
    }
    *node = nd;
    *st = r;
    return rc;
}

int dsm_read_dump(int node, const char *dir, dsm_node_state *st) {
    if (!st || node < 0 || node >= DSM_MAX_NP) return DSM_E_INVAL;
    char buf[DSM_DUMP_MAX + 2], path[512];
    if (dir) snprintf(path, sizeof path, "%s/core_%d_output.txt", dir, node);
    else snprintf(path, sizeof path, "core_%d_output.txt", node);         /* :831 */
    memset(st, 0, sizeof *st);
    FILE *f = fopen(path, "rb");
    if (!f) return DSM_E_IO;
    const size_t len = fread(buf, 1, sizeof buf, f);      /* one byte past the longest dump */
    const int bad = ferror(f);
    fclose(f);
    if (bad) return DSM_E_IO;
    int nd = -1;
    const int rc = dsm_parse_dump(buf, len, &nd, st);
    if (rc == DSM_OK && nd != node) {
        memset(st, 0, sizeof *st);
        return DSM_E_FORMAT;
    }
    return rc;
}

int dsm_format_issue_trace(const uint32_t *events, uint32_t n, char *buf, size_t cap) {
    if ((n && !events) || !buf) return DSM_E_INVAL;
    size_t k = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t e = events[i], ins = e & 0xFFFFu;
        const int w = snprintf(buf + k, cap - k, "Processor %u: instr type=%c, address=0x%02X, value=%u\n",
                               e >> 16, (ins >> 15) ? 'W' : 'R', (ins >> 8) & 0x7Fu, ins & 0xFFu);
        if (w < 0 || (size_t)w >= cap - k) return DSM_E_INVAL;                /* :596-597 */
        k += (size_t)w;
    }
    if (k < cap) buf[k] = 0;
    return (int)k;
}

static uint64_t fmix64(uint64_t z) {
    z ^= z >> 33; z *= 0xff51afd7ed558ccdULL;
    z ^= z >> 33; z *= 0xc4ceb9fe1a85ec53ULL;
    z ^= z >> 33;
    return z;
}

uint64_t dsm_node_hash(int node, const dsm_node_state *st, int nwords) {
    uint32_t w[16];
    memcpy(w, st, sizeof w);
    if (nwords > 16) nwords = 16;
    uint64_t h = 0x9E3779B97F4A7C15ULL * (uint64_t)(node + 1);
    for (int i = 0; i < nwords; ++i) h = fmix64(h ^ ((uint64_t)w[i] | ((uint64_t)i << 32)));
    return h;
}

/* one system's term of the aggregate's result digest: a fmix64 chain over the absolute
 * system id and the six result fields (position-sensitive, so a sum of terms pins every
 * system's result, and shards merge by addition) */
uint64_t dsm_result_digest(uint64_t sys_id, const dsm_sys_result *r) {
    uint64_t h = fmix64(sys_id * 0x9E3779B97F4A7C15ULL + 1u);
    h = fmix64(h ^ ((uint64_t)r->status | ((uint64_t)r->rounds << 32)));
    h = fmix64(h ^ ((uint64_t)r->msgs | ((uint64_t)r->instrs << 32)));
    h = fmix64(h ^ r->dump_hash);
    return fmix64(h ^ r->final_hash);
}

int dsm_aggregate_results(const dsm_sys_result *res, uint64_t n_sys, uint64_t first_sys,
                          dsm_aggregate *agg) {
    if (!agg || (n_sys && !res)) return DSM_E_INVAL;
    memset(agg, 0, sizeof *agg);
    for (uint64_t i = 0; i < n_sys; ++i) {
        const dsm_sys_result *r = &res[i];
        agg->systems++;
        agg->msgs += r->msgs;
        agg->instrs += r->instrs;
        agg->rounds += r->rounds;
        if (r->rounds > agg->max_rounds) agg->max_rounds = r->rounds;
        if ((r->status & 0xFFu) < 5u) agg->by_status[r->status & 0xFFu]++;
        agg->sum_dump_hash += r->dump_hash;
        agg->sum_final_hash += r->final_hash;
        agg->result_digest += dsm_result_digest(first_sys + i, r);
    }
    return DSM_OK;
}

/* ---- outcome census (include/dsm.h): the plain reference of csrc/dsm_census.hip ---------- */

/* A fmix64 chain in the style of dsm_result_digest, seeded by the kind instead of the system
 * id.  fmix64 is a bijection with fmix64(0) == 0, so the chain ends in 0 exactly when its last
 * input equals the chain so far; that one value is mapped to 1 (0 marks an empty slot). */
uint64_t dsm_outcome_key(int kind, const dsm_sys_result *r) {
    uint64_t h = fmix64((uint64_t)(kind + 1) * 0x9E3779B97F4A7C15ULL + 1u);
    if (kind == DSM_CENSUS_FULL) {
        h = fmix64(h ^ ((uint64_t)r->status | ((uint64_t)r->rounds << 32)));
        h = fmix64(h ^ ((uint64_t)r->msgs | ((uint64_t)r->instrs << 32)));
    } else {
        h = fmix64(h ^ (uint64_t)r->status);
    }
    h = fmix64(h ^ r->dump_hash);
    if (kind != DSM_CENSUS_DUMPS) h = fmix64(h ^ r->final_hash);
    return h ? h : 1u;
}

static int census_cap_ok(uint32_t cap) {
    return cap >= DSM_CENSUS_MIN_CAP && cap <= DSM_CENSUS_MAX_CAP && (cap & (cap - 1u)) == 0u;
}

/* count systems of `key`, the lowest of them ~inv_first, into the table; 0 when the key found
 * neither its slot nor a free one within cap probes */
static int census_add(uint64_t *census, uint32_t cap, uint64_t key, uint64_t count, uint64_t inv_first) {
    uint64_t s = key & (cap - 1u);
    for (uint32_t p = 0; p < cap; ++p, s = (s + 1u) & (cap - 1u)) {
        uint64_t *slot = census + 4 + 4 * s;
        if (slot[0] == 0) {
            slot[0] = key;
            census[1]++;
        }
        if (slot[0] == key) {
            slot[1] += count;
            if (inv_first > slot[2]) slot[2] = inv_first;
            return 1;
        }
    }
    return 0;
}

int dsm_census_results(const dsm_sys_result *res, uint64_t n_sys, uint64_t first_sys, int kind,
                       uint64_t *census, uint32_t cap) {
    if (!census || (n_sys && !res) || !census_cap_ok(cap)) return DSM_E_INVAL;
    if (kind != DSM_CENSUS_DUMPS && kind != DSM_CENSUS_FINAL && kind != DSM_CENSUS_FULL) return DSM_E_INVAL;
    memset(census, 0, DSM_CENSUS_WORDS(cap) * sizeof(uint64_t));
    for (uint64_t i = 0; i < n_sys; ++i) (void)dsm_census_insert(census, cap, dsm_outcome_key(kind, &res[i]), first_sys + i);
    return DSM_OK;
}

/* one system: the update dsm_census_results loops over */
int dsm_census_insert(uint64_t *census, uint32_t cap, uint64_t key, uint64_t sys_id) {
    if (!census || !census_cap_ok(cap) || key == 0) return DSM_E_INVAL;
    census[0]++;
    if (!census_add(census, cap, key, 1, ~sys_id)) census[2]++;
    return DSM_OK;
}

int dsm_census_merge(uint64_t *dst, const uint64_t *src, uint32_t cap) {
    if (!dst || !src || dst == src || !census_cap_ok(cap)) return DSM_E_INVAL;
    dst[0] += src[0];
    dst[2] += src[2];
    for (uint32_t s = 0; s < cap; ++s) {
        const uint64_t *slot = src + 4 + 4 * (uint64_t)s;
        if (slot[0] && !census_add(dst, cap, slot[0], slot[1], slot[2])) dst[2] += slot[1];
    }
    return DSM_OK;
}

static int outcome_cmp(const void *pa, const void *pb) {
    const dsm_outcome *a = (const dsm_outcome *)pa, *b = (const dsm_outcome *)pb;
    if (a->count != b->count) return a->count > b->count ? -1 : 1;
    return a->first_sys < b->first_sys ? -1 : (a->first_sys > b->first_sys ? 1 : 0);
}

int dsm_census_sorted(const uint64_t *census, uint32_t cap, dsm_outcome *out, uint64_t out_cap,
                      uint64_t *n) {
    if (!census || !n || (out_cap && !out) || !census_cap_ok(cap)) return DSM_E_INVAL;
    uint64_t k = 0;
    for (uint32_t s = 0; s < cap; ++s) k += census[4 + 4 * (uint64_t)s] != 0;
    *n = k;
    if (k == 0 || out_cap == 0) return DSM_OK;
    dsm_outcome *all = (dsm_outcome *)malloc((size_t)k * sizeof *all);
    if (!all) return DSM_E_NOMEM;
    k = 0;
    for (uint32_t s = 0; s < cap; ++s) {
        const uint64_t *slot = census + 4 + 4 * (uint64_t)s;
        if (!slot[0]) continue;
        all[k].key = slot[0];
        all[k].count = slot[1];
        all[k].first_sys = ~slot[2];
        ++k;
    }
    qsort(all, (size_t)k, sizeof *all, outcome_cmp);
    memcpy(out, all, (size_t)(k < out_cap ? k : out_cap) * sizeof *all);
    free(all);
    return DSM_OK;
}

int dsm_census_find(const uint64_t *census, uint32_t cap, uint64_t key, dsm_outcome *out) {
    if (!census || !census_cap_ok(cap) || key == 0) return DSM_E_INVAL;
    uint64_t s = key & (cap - 1u);
    for (uint32_t p = 0; p < cap; ++p, s = (s + 1u) & (cap - 1u)) {
        const uint64_t *slot = census + 4 + 4 * s;
        if (slot[0] == 0) return 0;                 /* the chain ends: slots are never freed */
        if (slot[0] != key) continue;
        if (out) {
            out->key = key;
            out->count = slot[1];
            out->first_sys = ~slot[2];
        }
        return 1;
    }
    return 0;
}

/* ---- coherence audit (include/dsm.h): the plain reference of csrc/dsm_audit.hip ---------- */

static const char *const audit_names[DSM_AUDIT_NCLASS] = {"MULTI_OWNER", "OWNER_AND_SHARER", "DIR_EM", "DIR_S",
                                                          "DIR_U", "STALE_VALUE", "BAD_RECORD"};

const char *dsm_audit_class_name(int bit) {
    return bit >= 0 && bit < DSM_AUDIT_NCLASS ? audit_names[bit] : NULL;
}

static int popcount8(uint32_t x) {
    int n = 0;
    for (; x; x &= x - 1u) ++n;
    return n;
}

/* one system: the np final records st[c * stride] -> its audit word */
static uint32_t audit_system(int np, const dsm_node_state *st, uint32_t stride) {
    const int na = DSM_MEM_SIZE * np;
    uint8_t me[DSM_MEM_SIZE * DSM_MAX_NP] = {0}, sh[DSM_MEM_SIZE * DSM_MAX_NP] = {0};
    uint8_t stale[DSM_MEM_SIZE * DSM_MAX_NP] = {0};
    uint32_t bad = 0, classes = 0, lines = 0, first = 0xFFu;
    for (int c = 0; c < np; ++c) {
        const dsm_node_state *r = st + (size_t)c * stride;
        for (int s = 0; s < DSM_CACHE_SIZE; ++s) {
            const int a = r->cache_addr[s], cs = r->cache_state[s];
            if (cs == 3 || a == 0xFF) continue;                       /* not held */
            if (cs > 3 || a >= na || (a & 3) != s) { ++bad; continue; }
            if (cs <= 1) me[a] |= (uint8_t)(1u << c);
            else sh[a] |= (uint8_t)(1u << c);
            if (cs != 0 && r->cache_value[s] != st[(size_t)(a >> 4) * stride].memory[a & 15]) stale[a] = 1;
        }
    }
    for (int a = 0; a < na; ++a) {
        const dsm_node_state *h = st + (size_t)(a >> 4) * stride;
        const uint32_t bv = h->dir_bv[a & 15], d = h->dir_state[a & 15], m = me[a], s = sh[a];
        uint32_t v = 0;
        if (popcount8(m) > 1) v |= 1u << DSM_AUDIT_MULTI_OWNER;
        if (m && s) v |= 1u << DSM_AUDIT_OWNER_AND_SHARER;
        if (d > 2) ++bad;
        else if (d == 0 && (bv != m || popcount8(m) != 1)) v |= 1u << DSM_AUDIT_DIR_EM;
        else if (d == 1 && (bv != s || s == 0 || m != 0)) v |= 1u << DSM_AUDIT_DIR_S;
        else if (d == 2 && (m | s)) v |= 1u << DSM_AUDIT_DIR_U;
        if (stale[a]) v |= 1u << DSM_AUDIT_STALE_VALUE;
        if (v) {
            classes |= v;
            if (lines++ == 0) first = (uint32_t)a;
        }
    }
    if (bad) classes |= 1u << DSM_AUDIT_BAD_RECORD;
    return classes | lines << 8 | first << 16 | bad << 24;
}

int dsm_audit_states(int np, const dsm_node_state *states, uint32_t state_stride, uint64_t n_sys,
                     uint64_t first_sys, uint32_t *words, dsm_audit *audit) {
    if ((np != 4 && np != 8) || state_stride == 0) return DSM_E_INVAL;
    if (n_sys && (!states || (!words && !audit))) return DSM_E_INVAL;
    if (audit) memset(audit, 0, sizeof *audit);
    for (uint64_t k = 0; k < n_sys; ++k) {
        const uint32_t w = audit_system(np, states + (size_t)k * (size_t)np * state_stride, state_stride);
        if (words) words[k] = w;
        if (!audit) continue;
        const uint64_t inv = ~(first_sys + k);
        audit->systems++;
        audit->lines += (w >> 8) & 0xFFu;
        audit->bad_items += w >> 24;
        if (!(w & 0x7Fu)) continue;
        audit->violating++;
        if (inv > audit->inv_first[7]) audit->inv_first[7] = inv;
        for (int b = 0; b < DSM_AUDIT_NCLASS; ++b) {
            if (!((w >> b) & 1u)) continue;
            audit->by_class[b]++;
            if (inv > audit->inv_first[b]) audit->inv_first[b] = inv;
        }
    }
    return DSM_OK;
}

int dsm_audit_merge(dsm_audit *dst, const dsm_audit *src) {
    if (!dst || !src || dst == src) return DSM_E_INVAL;
    dst->systems += src->systems;
    dst->violating += src->violating;
    dst->lines += src->lines;
    dst->bad_items += src->bad_items;
    for (int b = 0; b < 8; ++b) {
        dst->by_class[b] += src->by_class[b];
        if (src->inv_first[b] > dst->inv_first[b]) dst->inv_first[b] = src->inv_first[b];
    }
    for (int b = 0; b < 12; ++b) dst->reserved[b] += src->reserved[b];
    return DSM_OK;
}
