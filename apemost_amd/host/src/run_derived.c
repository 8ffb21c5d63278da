/* the derived file's parser, derived.bin reader and writer and the text files of the APEMOST_DUMP token `derived`
 * (run_derived.h); nothing here needs a device */
#include "run_derived.h"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "run_io.h"

#define alloc_or_die(count, size) run_alloc_or_die(count, size, "derived quantities")
#define read_or_die(p, size, count, f, path) run_read_or_die(p, size, count, f, path, "derived file")

#define RUN_DERIVED_MAGIC "APEMOSTD"
#define RUN_DERIVED_VERSION 1
#define NAME_MAX_LEN 200

/* the opcode names in the order of their numbers (include/apemost_hip.h) */
static const char *const op_names[APEMOST_DERIVED_N_OPCODES] = {
    "col", "const", "dup", "swap", "add", "sub", "mul", "div", "neg", "abs", "inv", "sqrt", "floor", "min", "max",
    "log", "exp", "sin", "cos", "atan2"};

static char *copy_text(const char *s, size_t len) {
    char *p = (char *)alloc_or_die(len + 1, 1);
    memcpy(p, s, len);
    p[len] = 0;
    return p;
}

/* a number in full, as Python's float() reads it too: no hexadecimal form */
static int parse_number(const char *tok, double *v) {
    char *end;
    if (*tok == 0 || strchr(tok, 'x') != NULL || strchr(tok, 'X') != NULL)
        return 0;
    *v = strtod(tok, &end);
    return *end == 0 && end != tok;
}

/* the column a name pushes, or -1 */
static int column_of(const char *tok, unsigned int n_par, const char *const *param_names) {
    unsigned int p;
    for (p = 0; p < n_par; p++)
        if (strcmp(tok, param_names[p]) == 0)
            return (int)p;
    if (strcmp(tok, "prob") == 0)
        return (int)n_par;
    if (strcmp(tok, "like") == 0)
        return (int)n_par + 1;
    return -1;
}

int run_derived_parse(const char *text, unsigned int n_par, const char *const *param_names, run_derived *r, char *message) {
    char *copy = copy_text(text, strlen(text)), *line = copy;
    unsigned int line_no = 0, p;
    int bad = 0;
    memset(r, 0, sizeof *r);
    message[0] = 0;
    r->n_par = n_par;
    r->names = (char **)alloc_or_die(APEMOST_DERIVED_MAX_COLUMNS, sizeof(char *));
    r->rpn = (char **)alloc_or_die(APEMOST_DERIVED_MAX_COLUMNS, sizeof(char *));
    r->row_names = (char **)alloc_or_die(n_par, sizeof(char *));
    r->code = (int32_t *)alloc_or_die((size_t)APEMOST_DERIVED_MAX_COLUMNS * APEMOST_DERIVED_MAX_CODE, sizeof(int32_t));
    r->start = (int32_t *)alloc_or_die(APEMOST_DERIVED_MAX_COLUMNS + 1, sizeof(int32_t));
    r->consts = (double *)alloc_or_die(APEMOST_DERIVED_MAX_CONSTS, sizeof(double));
    r->lo = (double *)alloc_or_die(APEMOST_DERIVED_MAX_COLUMNS, sizeof(double));
    r->hi = (double *)alloc_or_die(APEMOST_DERIVED_MAX_COLUMNS, sizeof(double));
    for (p = 0; p < n_par; p++)
        r->row_names[p] = copy_text(param_names[p], strlen(param_names[p]));
    while (line != NULL && !bad) {
        char *next = strchr(line, '\n'), *hash, *tok;
        char *rpn;
        int32_t *code;
        int32_t one[2];
        unsigned int n_tok = 0, len = 0, c;
        double lo = 0, hi = 0;
        if (next != NULL)
            *next++ = 0;
        line_no++;
        hash = strchr(line, '#');
        if (hash != NULL)
            *hash = 0;
        rpn = (char *)alloc_or_die(strlen(line) + 2, 1);
        code = r->code + r->start[r->n_col];
        for (tok = strtok(line, " \t\r"); tok != NULL && !bad; tok = strtok(NULL, " \t\r"), n_tok++) {
            if (n_tok == 0) {
                if (r->n_col == APEMOST_DERIVED_MAX_COLUMNS) {
                    sprintf(message, "line %u: more than %d columns", line_no, APEMOST_DERIVED_MAX_COLUMNS);
                    bad = 1;
                } else if (strlen(tok) > NAME_MAX_LEN || strchr(tok, '/') != NULL) {
                    sprintf(message, "line %u: the name '%.40s' is longer than %d characters or holds a '/'", line_no, tok,
                            NAME_MAX_LEN);
                    bad = 1;
                } else {
                    for (c = 0; c < r->n_col && !bad; c++)
                        if (strcmp(r->names[c], tok) == 0) {
                            sprintf(message, "line %u: a second column named '%.200s'", line_no, tok);
                            bad = 1;
                        }
                    if (!bad)
                        r->names[r->n_col] = copy_text(tok, strlen(tok));
                }
            } else if (n_tok <= 2) {
                if (!parse_number(tok, n_tok == 1 ? &lo : &hi)) {
                    sprintf(message, "line %u: '%.100s' is not a number (name lo hi tokens ...)", line_no, tok);
                    bad = 1;
                }
            } else {
                int32_t word = -1;
                double v;
                int col = column_of(tok, n_par, param_names), op;
                if (col >= 0)
                    word = APEMOST_DERIVED_COL | (col << 8);
                for (op = APEMOST_DERIVED_DUP; word < 0 && op < APEMOST_DERIVED_N_OPCODES; op++)
                    if (strcmp(tok, op_names[op]) == 0)
                        word = op;
                if (word < 0 && parse_number(tok, &v)) {
                    unsigned int k;
                    for (k = 0; k < r->n_const; k++) /* equal bit patterns share a slot */
                        if (memcmp(&r->consts[k], &v, sizeof v) == 0)
                            break;
                    if (k == APEMOST_DERIVED_MAX_CONSTS) {
                        sprintf(message, "line %u: more than %d different constants", line_no, APEMOST_DERIVED_MAX_CONSTS);
                        bad = 1;
                        break;
                    }
                    if (k == r->n_const)
                        r->consts[r->n_const++] = v;
                    word = APEMOST_DERIVED_CONST | (int32_t)(k << 8);
                }
                if (word < 0) {
                    sprintf(message, "line %u: token '%.100s' is neither a column, a number nor an operation", line_no, tok);
                    bad = 1;
                } else if (len == APEMOST_DERIVED_MAX_CODE) {
                    sprintf(message, "line %u: more than %d instructions", line_no, APEMOST_DERIVED_MAX_CODE);
                    bad = 1;
                } else {
                    code[len++] = word;
                    if (rpn[0] != 0)
                        strcat(rpn, " ");
                    strcat(rpn, tok);
                }
            }
        }
        if (!bad && n_tok > 0) {
            if (n_tok < 4) {
                sprintf(message, "line %u: expected `name lo hi` and at least one token", line_no);
                bad = 1;
            } else if (!(lo < hi) || !(lo - lo == 0) || !(hi - hi == 0) || !((hi - lo) - (hi - lo) == 0)) {
                sprintf(message, "line %u: range [%g, %g] invalid", line_no, lo, hi);
                bad = 1;
            } else {
                one[0] = 0;
                one[1] = (int32_t)len;
                if (apemost_hip_derived_check((int32_t)n_par, 1, code, one, (int32_t)r->n_const, NULL) != APEMOST_HIP_OK) {
                    sprintf(message, "line %u: %.300s", line_no, apemost_hip_last_error());
                    bad = 1;
                }
            }
        }
        if (!bad && n_tok > 0) {
            r->lo[r->n_col] = lo;
            r->hi[r->n_col] = hi;
            r->rpn[r->n_col] = rpn;
            r->start[r->n_col + 1] = r->start[r->n_col] + (int32_t)len;
            r->n_col++;
        } else
            free(rpn);
        line = next;
    }
    free(copy);
    if (bad)
        return (int)line_no;
    if (r->n_col == 0) {
        sprintf(message, "no column");
        return -1;
    }
    return 0;
}

void run_derived_alloc(run_derived *r) {
    const size_t nc = r->n_col;
    r->hist = (uint64_t *)alloc_or_die(nc * r->nbins, sizeof(uint64_t));
    r->batch = (double *)alloc_or_die(nc * (size_t)(r->max_batches + 1), sizeof(double));
    r->nonfinite = (uint64_t *)alloc_or_die(nc, sizeof(uint64_t));
    r->vmin = (double *)alloc_or_die(nc, sizeof(double));
    r->vmax = (double *)alloc_or_die(nc, sizeof(double));
    r->origin = (double *)alloc_or_die(nc, sizeof(double));
    r->sum = (double *)alloc_or_die(nc, sizeof(double));
    r->cross = (double *)alloc_or_die(run_tri_count(r->n_col), sizeof(double));
    r->counts = (uint64_t *)alloc_or_die((size_t)r->n_pairs * r->nbins * r->nbins, sizeof(uint64_t));
}

void run_derived_free(run_derived *r) {
    unsigned int c;
    for (c = 0; c < r->n_col && r->names != NULL; c++) {
        free(r->names[c]);
        free(r->rpn[c]);
    }
    for (c = 0; c < r->n_par && r->row_names != NULL; c++)
        free(r->row_names[c]);
    free(r->names);
    free(r->rpn);
    free(r->row_names);
    free(r->code);
    free(r->start);
    free(r->consts);
    free(r->lo);
    free(r->hi);
    free(r->pairs);
    free(r->hist);
    free(r->batch);
    free(r->nonfinite);
    free(r->vmin);
    free(r->vmax);
    free(r->origin);
    free(r->sum);
    free(r->cross);
    free(r->counts);
    memset(r, 0, sizeof *r);
}

static char *read_string(FILE *f, const char *path) {
    uint32_t len;
    char *s;
    read_or_die(&len, sizeof len, 1, f, path);
    if (len > (1u << 20)) {
        fprintf(stderr, "%s: not a derived file of version %d\n", path, RUN_DERIVED_VERSION);
        exit(1);
    }
    s = (char *)alloc_or_die((size_t)len + 1, 1);
    read_or_die(s, 1, len, f, path);
    return s;
}

static void write_string(FILE *f, const char *s) {
    const uint32_t len = (uint32_t)strlen(s);
    fwrite(&len, sizeof len, 1, f);
    fwrite(s, 1, len, f);
}

int run_derived_read(const char *path, run_derived *r) {
    FILE *f = fopen(path, "rb");
    char magic[8];
    uint32_t u32[6], n_names, c;
    uint64_t u64[5];
    int32_t chain;
    if (f == NULL)
        return -1;
    memset(r, 0, sizeof *r);
    read_or_die(magic, 1, 8, f, path);
    read_or_die(u32, sizeof(uint32_t), 6, f, path);
    read_or_die(u64, sizeof(uint64_t), 5, f, path);
    if (memcmp(magic, RUN_DERIVED_MAGIC, 8) != 0 || u32[0] != RUN_DERIVED_VERSION || u32[1] != 1 || u32[2] < 1 ||
        u32[2] > APEMOST_DERIVED_MAX_COLUMNS || u32[3] < 1 || u32[3] > 512 || u32[4] > u32[2] * (u32[2] - 1) / 2 ||
        u32[5] > 65535 || u64[2] < 1 || u64[3] > ((uint64_t)1 << 40) || u64[4] != run_batches_closed(u64[0], u64[2]) ||
        u64[4] > u64[3]) {
        fprintf(stderr, "%s: not a derived file of version %d and one kept chain\n", path, RUN_DERIVED_VERSION);
        exit(1);
    }
    r->n_col = u32[2];
    r->nbins = u32[3];
    r->n_pairs = u32[4];
    r->n_par = u32[5];
    r->n = u64[0];
    r->thin = u64[1];
    r->bs = u64[2];
    r->max_batches = u64[3];
    r->pairs = (int32_t *)alloc_or_die((size_t)r->n_pairs * 2, sizeof(int32_t));
    r->lo = (double *)alloc_or_die(r->n_col, sizeof(double));
    r->hi = (double *)alloc_or_die(r->n_col, sizeof(double));
    r->names = (char **)alloc_or_die(r->n_col, sizeof(char *));
    r->rpn = (char **)alloc_or_die(r->n_col, sizeof(char *));
    r->row_names = (char **)alloc_or_die(r->n_par, sizeof(char *));
    read_or_die(&chain, sizeof chain, 1, f, path);
    read_or_die(r->pairs, sizeof(int32_t), (size_t)r->n_pairs * 2, f, path);
    read_or_die(r->lo, sizeof(double), r->n_col, f, path);
    read_or_die(r->hi, sizeof(double), r->n_col, f, path);
    for (c = 0; c < r->n_col; c++) {
        r->names[c] = read_string(f, path);
        r->rpn[c] = read_string(f, path);
    }
    read_or_die(&n_names, sizeof n_names, 1, f, path);
    if (n_names != r->n_par || chain != 0) {
        fprintf(stderr, "%s: not a derived file of version %d and one kept chain\n", path, RUN_DERIVED_VERSION);
        exit(1);
    }
    for (c = 0; c < r->n_par; c++)
        r->row_names[c] = read_string(f, path);
    run_derived_alloc(r);
    read_or_die(r->hist, sizeof(uint64_t), (size_t)r->n_col * r->nbins, f, path);
    read_or_die(r->batch, sizeof(double), (size_t)r->n_col * (size_t)(r->max_batches + 1), f, path);
    read_or_die(r->nonfinite, sizeof(uint64_t), r->n_col, f, path);
    read_or_die(r->vmin, sizeof(double), r->n_col, f, path);
    read_or_die(r->vmax, sizeof(double), r->n_col, f, path);
    read_or_die(r->origin, sizeof(double), r->n_col, f, path);
    read_or_die(r->sum, sizeof(double), r->n_col, f, path);
    read_or_die(r->cross, sizeof(double), run_tri_count(r->n_col), f, path);
    read_or_die(r->counts, sizeof(uint64_t), (size_t)r->n_pairs * r->nbins * r->nbins, f, path);
    fclose(f);
    return 0;
}

void run_derived_write(const char *path, const run_derived *r) {
    FILE *f = run_open_or_die(path, "wb");
    uint32_t u32[6], c;
    uint64_t u64[5];
    const int32_t chain = 0;
    u32[0] = RUN_DERIVED_VERSION;
    u32[1] = 1;
    u32[2] = r->n_col;
    u32[3] = r->nbins;
    u32[4] = r->n_pairs;
    u32[5] = r->n_par;
    u64[0] = r->n;
    u64[1] = r->thin;
    u64[2] = r->bs;
    u64[3] = r->max_batches;
    u64[4] = run_batches_closed(r->n, r->bs);
    fwrite(RUN_DERIVED_MAGIC, 1, 8, f);
    fwrite(u32, sizeof(uint32_t), 6, f);
    fwrite(u64, sizeof(uint64_t), 5, f);
    fwrite(&chain, sizeof chain, 1, f);
    fwrite(r->pairs, sizeof(int32_t), (size_t)r->n_pairs * 2, f);
    fwrite(r->lo, sizeof(double), r->n_col, f);
    fwrite(r->hi, sizeof(double), r->n_col, f);
    for (c = 0; c < r->n_col; c++) {
        write_string(f, r->names[c]);
        write_string(f, r->rpn[c]);
    }
    fwrite(&r->n_par, sizeof(uint32_t), 1, f);
    for (c = 0; c < r->n_par; c++)
        write_string(f, r->row_names[c]);
    fwrite(r->hist, sizeof(uint64_t), (size_t)r->n_col * r->nbins, f);
    fwrite(r->batch, sizeof(double), (size_t)r->n_col * (size_t)(r->max_batches + 1), f);
    fwrite(r->nonfinite, sizeof(uint64_t), r->n_col, f);
    fwrite(r->vmin, sizeof(double), r->n_col, f);
    fwrite(r->vmax, sizeof(double), r->n_col, f);
    fwrite(r->origin, sizeof(double), r->n_col, f);
    fwrite(r->sum, sizeof(double), r->n_col, f);
    fwrite(r->cross, sizeof(double), run_tri_count(r->n_col), f);
    fwrite(r->counts, sizeof(uint64_t), (size_t)r->n_pairs * r->nbins * r->nbins, f);
    run_close_or_die(f, path);
}

/* mean = origin + sum / n; sd = sqrt((cross_cc - sum^2 / n) / (n - 1)); mcse = batch_means_error() about that mean:
 * apemost_amd/derived.py, operation for operation */
void run_derived_write_text(const run_derived *r) {
    const double n = (double)r->n, n1 = n - 1.0;
    const uint64_t nb = run_batches_closed(r->n, r->bs);
    FILE *f = run_open_or_die("derived.txt", "w");
    unsigned int c, b;
    uint64_t k;
    size_t diag = 0;
    for (c = 0; c < r->n_col; c++) {
        const double part = r->sum[c] / n, mean = r->origin[c] + part;
        const double sq = r->sum[c] * r->sum[c], sq_n = sq / n, diff = r->cross[diag] - sq_n, var = diff / n1;
        const double *batch = r->batch + (size_t)c * (size_t)(r->max_batches + 1);
        const uint64_t *hist = r->hist + (size_t)c * r->nbins;
        double err = 0, mcse, total = 0, scale;
        char name[NAME_MAX_LEN + 32];
        FILE *h;
        for (k = 0; k < nb; k++) {
            const double m = batch[k] / (double)r->bs, d = m - mean, d2 = d * d;
            err += d2;
        }
        mcse = (nb > 0 && err >= 0) ? sqrt(err / (double)nb) : sqrt(-1.0);
        fprintf(f, "%s\t%lu\t", r->names[c], (unsigned long)r->n);
        run_print_values(f, 5, mean, sqrt(var), mcse, r->vmin[c], r->vmax[c]);
        fprintf(f, "\t%lu\n", (unsigned long)r->nonfinite[c]);
        diag += r->n_col - c; /* (c, c) of the row-major upper triangle */
        /* counts * (hi - lo) / nbins / total, as analyse scales a parameter's histogram */
        for (b = 0; b < r->nbins; b++)
            total += (double)hist[b];
        scale = (r->hi[c] - r->lo[c]) / r->nbins / total;
        sprintf(name, "%s.histogram", r->names[c]);
        h = run_open_or_die(name, "w");
        for (b = 0; b < r->nbins; b++) {
            fprintf(h, "%.15e %.15e ", run_summary_edge(r->lo[c], r->hi[c], b, r->nbins),
                    run_summary_edge(r->lo[c], r->hi[c], b + 1, r->nbins));
            run_print_value(h, (double)hist[b] * scale);
            fprintf(h, "\n");
        }
        run_close_or_die(h, name);
    }
    run_close_or_die(f, "derived.txt");
}
