// assoc.cpp — `pgen-hip assoc` (pfile.h, Pfile::output_assoc): the value files, the complete cases, the design (stats.h), one pass
// of the block loop (block_loop.h) with the linear or the logistic counter, and the lines.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>

#include "block_loop.h"
#include "stats.h"

namespace pgenhost {

namespace {

// assoc's counter: per block the rows' genotype counts and their per-code sums of every value column (Q's columns, then the
// residualised phenotypes; uploaded once per shard), sixteen columns per launch; both come back block by block.  Group g's sums of
// a block are bv x cg x 4 doubles behind those of the groups before it.
struct AssocCounter : Counter {
    size_t C, bv;                     // value columns, rows of a full block
    std::vector<uint32_t> &counts;    // 4 per kept variant
    std::vector<double> &sums;        // per kept variant C x 4
    const double *d_values;
    uint32_t *d_gc, *h_gc;
    double *d_sums, *h_sums;
    void launch(const BlockRows &b, size_t, uint32_t nv, uint32_t, bool) const
    {
        genotype_counts(b, nv, d_gc);
        column_groups(C, PGENHIP_VSUM_MAX_COLUMNS, [&](size_t c0, size_t cg) {
            launch_rows(b, NAMED(pgenhip_variant_sums), NAMED(pgenhip_variant_sums_at), nv, d_values + c0, C, (uint32_t)cg, d_sums + bv * 4 * c0, PGENHIP_VSUM_AUTO);
        });
    }
    void copy(pgenhip_ctx *ctx, size_t nv) const
    {
        check(pgenhip_memcpy_d2h(ctx, h_gc, d_gc, nv * 16), "D2H counts");
        column_groups(C, PGENHIP_VSUM_MAX_COLUMNS, [&](size_t c0, size_t cg) {
            check(pgenhip_memcpy_d2h(ctx, h_sums + bv * 4 * c0, d_sums + bv * 4 * c0, nv * cg * 4 * sizeof(double)), "D2H sums");
        });
    }
    void collect(size_t b0, size_t nv) const
    {
        std::memcpy(counts.data() + 4 * b0, h_gc, nv * 16);
        column_groups(C, PGENHIP_VSUM_MAX_COLUMNS, [&](size_t c0, size_t cg) {
            const double *src = h_sums + bv * 4 * c0;
            for (size_t j = 0; j < nv; j++) std::memcpy(sums.data() + ((b0 + j) * C + c0) * 4, src + j * cg * 4, cg * 4 * sizeof(double));
        });
    }
};

// assoc --logistic's counter: per block the rows' genotype counts come back at once (a row's code table holds its mean dosage), the
// tables go up, and one pgenhip_variant_logistic per phenotype follows; the genotype's coefficient and standard error and the status
// word of every (phenotype, row) come back block by block.  The design (n x m), the 0 / 1 phenotypes (P x n) and the null models'
// coefficients (P x m) are uploaded once per shard.
struct LogitCounter : Counter {
    size_t P, m, n, bv;
    const AssocOptions &ao;
    std::vector<uint32_t> &counts;    // 4 per kept variant
    std::vector<double> &beta, &se;   // P per kept variant
    std::vector<uint32_t> &status;    // P per kept variant
    const double *d_design, *d_y, *d_start;
    uint32_t *d_gc, *h_gc;
    double *d_tab, *h_tab;            // 4 per row
    double *d_coef, *h_coef;          // P x bv x (m + 1)
    double *d_se, *h_se;              // P x bv
    uint32_t *d_status, *h_status;    // P x bv
    void launch(const BlockRows &b, size_t, uint32_t nv, uint32_t, bool) const
    {
        genotype_counts_now(b, nv, d_gc, h_gc);
        for (uint32_t j = 0; j < nv; j++) {
            double *t = h_tab + 4 * (size_t)j;
            t[0] = 0.0, t[1] = 1.0, t[2] = 2.0;
            t[3] = ao.mean_imputation ? stats::mean_dosage(h_gc + 4 * j) : std::nan("");
        }
        check(pgenhip_memcpy_h2d(b.ctx, d_tab, h_tab, (size_t)nv * 4 * sizeof(double)), "H2D code tables");
        for (size_t p = 0; p < P; p++)
            launch_rows(b, NAMED(pgenhip_variant_logistic), NAMED(pgenhip_variant_logistic_at), nv, d_tab, d_design, (uint64_t)m, (uint32_t)m,
                        d_y + p * n, d_start + p * m, ao.max_iter, ao.tol, d_coef + p * bv * (m + 1), (uint64_t)(m + 1), d_se + p * bv,
                        d_status + p * bv, PGENHIP_LOGIT_AUTO);
    }
    void copy(pgenhip_ctx *ctx, size_t nv) const
    {
        for (size_t p = 0; p < P; p++) {
            check(pgenhip_memcpy_d2h(ctx, h_coef + p * bv * (m + 1), d_coef + p * bv * (m + 1), nv * (m + 1) * sizeof(double)), "D2H coefficients");
            check(pgenhip_memcpy_d2h(ctx, h_se + p * bv, d_se + p * bv, nv * sizeof(double)), "D2H standard errors");
            check(pgenhip_memcpy_d2h(ctx, h_status + p * bv, d_status + p * bv, nv * sizeof(uint32_t)), "D2H status words");
        }
    }
    void collect(size_t b0, size_t nv) const
    {
        std::memcpy(counts.data() + 4 * b0, h_gc, nv * 16);
        for (size_t p = 0; p < P; p++)
            for (size_t j = 0; j < nv; j++) {
                beta[(b0 + j) * P + p] = h_coef[(p * bv + j) * (m + 1) + m];
                se[(b0 + j) * P + p] = h_se[p * bv + j];
                status[(b0 + j) * P + p] = h_status[p * bv + j];
            }
    }
};

// What assoc prepares before any arithmetic, in two steps because the selection is evaluated between them (so that a bad value file
// is reported before a bad query): read_tables fills the files' part, complete_cases the rest from the selection
struct AssocPrep {
    ValueTable ph, cv;
    std::vector<size_t> pcol;                  // the chosen phenotype columns of ph
    std::vector<stats::BinaryCoding> coding;   // --logistic: how each of them codes case / control
    size_t P = 0, ncov = 0, m = 0, n = 0;      // phenotypes, covariates, 1 + ncov, complete cases
    size_t col[5];                             // kVariantColumns in the .pvar
    std::vector<double> y, x;                  // n x P phenotypes, n x ncov covariates
    const std::string &pheno_name(size_t p) const { return ph.names[pcol[p]]; }
};

// both value files, the chosen phenotype columns, and --logistic's checks of the covariate count and the case/control coding
AssocPrep read_tables(const AssocOptions &aopt)
{
    AssocPrep a;
    a.ph = read_value_table(aopt.pheno_file);
    if (!aopt.covar_file.empty()) a.cv = read_value_table(aopt.covar_file);
    const ValueTable &ph = a.ph;
    if (aopt.pheno_names.empty()) {
        for (size_t c = 0; c < ph.names.size(); c++) a.pcol.push_back(c);
    } else {
        for (const std::string &name : aopt.pheno_names) {
            const size_t c = std::find(ph.names.begin(), ph.names.end(), name) - ph.names.begin();
            if (c == ph.names.size()) throw PfileError(aopt.pheno_file + " line 1: no phenotype column named '" + name + "'");
            a.pcol.push_back(c);
        }
    }
    a.P = a.pcol.size();
    a.ncov = a.cv.names.size();
    a.m = 1 + a.ncov;
    a.coding.assign(a.P, stats::BinaryCoding::kNone);
    if (aopt.logistic) {
        if (a.m > PGENHIP_LOGIT_MAX_COVARIATES)
            throw PfileError(aopt.covar_file + ": " + std::to_string(a.ncov) + " covariates; assoc --logistic takes " + std::to_string(PGENHIP_LOGIT_MAX_COVARIATES - 1) + " at most");
        for (size_t p = 0; p < a.P; p++) {
            a.coding[p] = stats::binary_coding(ph.x.data() + a.pcol[p], ph.iids.size(), ph.names.size());
            if (a.coding[p] == stats::BinaryCoding::kNone)
                throw PfileError(aopt.pheno_file + ": phenotype " + a.pheno_name(p) + " is not a case/control column (every value 1 or 2 with a 2 present, or every value 0 or 1)");
        }
    }
    return a;
}

// the .pvar columns of the lines, and the selection's samples reduced to the complete cases: a kept sample stays only with every
// chosen phenotype and every covariate; their values in a.y and a.x, and the two errors about how many there are
void complete_cases(const Pfile &pf, const AssocOptions &aopt, AssocPrep &a, Pfile::Selection &sel, OutputStats &st)
{
    const ValueTable &ph = a.ph, &cv = a.cv;
    const size_t P = a.P, ncov = a.ncov, m = a.m;
    const size_t iid = iid_column(pf, sel.sam_header);
    pvar_columns(pf, sel.var_header, kVariantColumns, a.col);

    std::map<std::string, size_t> ph_row, cv_row;
    for (size_t i = 0; i < ph.iids.size(); i++) ph_row.emplace(ph.iids[i], i);
    for (size_t i = 0; i < cv.iids.size(); i++) cv_row.emplace(cv.iids[i], i);
    Pfile::IdxRecords stay;
    for (auto &sr : sel.sam_idx_rcs) {
        const auto pi = ph_row.find(sr.second.at(iid));
        const auto ci = ncov ? cv_row.find(sr.second.at(iid)) : cv_row.end();
        bool complete = pi != ph_row.end() && (!ncov || ci != cv_row.end());
        for (size_t p = 0; complete && p < P; p++) complete = !std::isnan(ph.x[pi->second * ph.names.size() + a.pcol[p]]);
        for (size_t c = 0; complete && c < ncov; c++) complete = !std::isnan(cv.x[ci->second * ncov + c]);
        if (!complete) continue;
        for (size_t p = 0; p < P; p++) a.y.push_back(ph.x[pi->second * ph.names.size() + a.pcol[p]]);
        for (size_t c = 0; c < ncov; c++) a.x.push_back(cv.x[ci->second * ncov + c]);
        stay.push_back(std::move(sr));
    }
    st.assoc_dropped = sel.sam_idx_rcs.size() - stay.size();
    sel.sam_idx_rcs = std::move(stay);
    const size_t n = a.n = sel.sam_idx_rcs.size();
    if (n == 0) throw PfileError("no kept sample has every chosen phenotype of " + aopt.pheno_file + (ncov ? " and every covariate of " + aopt.covar_file : std::string()));
    if (n < m + 2)
        throw PfileError("too few samples: " + std::to_string(n) + " complete samples leave " + std::to_string((long long)n - (long long)m - 1) +
                         " degrees of freedom for an intercept, " + std::to_string(ncov) + " covariates and the genotype");
}

// The design step, from the complete cases.  Linear: the value columns, n x (m + P): Q's m columns, then the residualised
// phenotypes.  Logistic: n x m, Q's columns scaled by sqrt(n); the phenotypes as 0 / 1, P x n; the null models' coefficients, P x m
struct AssocFit {
    stats::AssocDesign design;            // linear
    std::vector<double> xq, y01, start;   // logistic
};
AssocFit design_step(const AssocOptions &aopt, const AssocPrep &a)
{
    AssocFit f;
    const size_t P = a.P, m = a.m, n = a.n;
    const size_t c = aopt.logistic ? stats::logistic_design(a.x, n, a.ncov, f.xq) : stats::assoc_design(a.x, a.y, n, a.ncov, P, f.design);
    if (c != stats::kNoColumn)
        throw PfileError(aopt.covar_file + ": covariate " + (c ? a.cv.names[c - 1] : std::string("(intercept)")) + " is collinear with the intercept and the covariates before it");
    if (!aopt.logistic) return f;
    f.y01.resize(P * n);
    f.start.resize(P * m);
    for (size_t p = 0; p < P; p++) {
        size_t cases = 0;
        for (size_t k = 0; k < n; k++) cases += (f.y01[p * n + k] = stats::binary_value(a.y[k * P + p], a.coding[p])) != 0.0;
        if (cases == 0 || cases == n)
            throw PfileError(aopt.pheno_file + ": phenotype " + a.pheno_name(p) + " has no " + (cases ? "control" : "case") + " among the " + std::to_string(n) + " complete samples");
        const stats::LogisticNull null = stats::logistic_null(f.xq, n, m, f.y01.data() + p * n, (int)PGENHIP_LOGIT_MAX_ITER, 1e-12);
        if (!null.converged)
            throw PfileError(aopt.pheno_file + ": the null model of phenotype " + a.pheno_name(p) + " (intercept and covariates alone) did not converge: the covariates separate it");
        std::copy(null.beta.begin(), null.beta.end(), f.start.begin() + p * m);
    }
    return f;
}

}  // namespace

ValueTable read_value_table(const std::string &path)
{
    ValueTable vt;
    KeyedRows t = read_keyed_rows(path, 1, "a value file has an IID column and at least one value column", "IID",
                                  [&](const std::string &cell, const std::string &name, const std::string &where) {
        if (cell.empty() || cell == "NA" || cell == "nan") {
            vt.x.push_back(std::nan(""));
            return;
        }
        char *end = nullptr;
        const double x = std::strtod(cell.c_str(), &end);
        if (*end != '\0' || !std::isfinite(x)) throw PfileError(where + ": value '" + cell + "' of column " + name + " is not a finite number, NA or nan");
        vt.x.push_back(x);
    });
    vt.names = std::move(t.names);
    vt.iids = std::move(t.lead[0]);
    return vt;
}

OutputStats Pfile::output_assoc(const std::optional<std::string> &sam_query, const std::optional<std::string> &var_query,
                                const AssocOptions &aopt, const std::string &filename, const OutputOptions &opt) const
{
    OutputStats st;
    const double t0 = now_s();
    AssocPrep a = read_tables(aopt);
    AssocFit fit;
    // the rest of the preparation and the design step belong to seconds_filter, and run before check_selection
    const Opening o = open_selection(*this, sam_query, var_query, opt, st, false, [&](Selection &sel) {
        complete_cases(*this, aopt, a, sel, st);
        fit = design_step(aopt, a);
    }, t0);
    const stats::AssocDesign &design = fit.design;
    const std::vector<double> &xq = fit.xq, &y01 = fit.y01, &start = fit.start;
    const IdxRecords &vars = o.sel.var_idx_rcds;
    const size_t P = a.P, m = a.m, C = m + P, V = o.V, n = a.n;

    // what comes back per kept variant: its 4 counts; linear, C x 4 sums; logistic, P coefficients, standard errors and status words
    std::vector<uint32_t> counts(4 * V, 0u), status(aopt.logistic ? V * P : 0, 0u);
    std::vector<double> sums(aopt.logistic ? 0 : V * C * 4, 0.0), beta(status.size(), 0.0), se(status.size(), 0.0);
    const double t_body = now_s();
    static const char *const kNoDevice = "no HIP device: the assoc path has no CPU fallback";
    // without a kept variant: the header alone, and no device is touched
    if (V != 0 && aopt.logistic) {
        count_blocks(*this, vars, o.kept, opt, kNoDevice, st, [&](DeviceCtx &ctx, uint64_t bv) {
            const size_t b = (size_t)bv;
            double *d_design = ctx.device<double>(n * m * sizeof(double), "device design");
            double *d_y = ctx.device<double>(P * n * sizeof(double), "device phenotypes");
            double *d_start = ctx.device<double>(P * m * sizeof(double), "device null models");
            check(pgenhip_memcpy_h2d(ctx.get(), d_design, xq.data(), n * m * sizeof(double)), "H2D design");
            check(pgenhip_memcpy_h2d(ctx.get(), d_y, y01.data(), P * n * sizeof(double)), "H2D phenotypes");
            check(pgenhip_memcpy_h2d(ctx.get(), d_start, start.data(), P * m * sizeof(double)), "H2D null models");
            check(pgenhip_wait(ctx.get()), "pgenhip_wait");
            return LogitCounter{{}, P, m, n, b, aopt, counts, beta, se, status, d_design, d_y, d_start,
                                ctx.device<uint32_t>(16 * b, "device variant counts"), ctx.pinned<uint32_t>(16 * b, "pinned variant counts"),
                                ctx.device<double>(b * 4 * sizeof(double), "device code tables"), ctx.pinned<double>(b * 4 * sizeof(double), "pinned code tables"),
                                ctx.device<double>(P * b * (m + 1) * sizeof(double), "device coefficients"), ctx.pinned<double>(P * b * (m + 1) * sizeof(double), "pinned coefficients"),
                                ctx.device<double>(P * b * sizeof(double), "device standard errors"), ctx.pinned<double>(P * b * sizeof(double), "pinned standard errors"),
                                ctx.device<uint32_t>(P * b * sizeof(uint32_t), "device status words"), ctx.pinned<uint32_t>(P * b * sizeof(uint32_t), "pinned status words")};
        });
    } else if (V != 0) {
        count_blocks(*this, vars, o.kept, opt, kNoDevice, st, [&](DeviceCtx &ctx, uint64_t bv) {
            const size_t b = (size_t)bv;
            double *d_values = ctx.device<double>(n * C * sizeof(double), "device values");
            check(pgenhip_memcpy_h2d(ctx.get(), d_values, design.values.data(), n * C * sizeof(double)), "H2D values");
            check(pgenhip_wait(ctx.get()), "pgenhip_wait");
            return AssocCounter{{}, C, b, counts, sums, d_values,
                                ctx.device<uint32_t>(16 * b, "device variant counts"), ctx.pinned<uint32_t>(16 * b, "pinned variant counts"),
                                ctx.device<double>(b * C * 4 * sizeof(double), "device sums"), ctx.pinned<double>(b * C * 4 * sizeof(double), "pinned sums")};
        });
    }

    std::string text = "#CHROM\tPOS\tID\tREF\tALT\tA1\tPHENO\tOBS_CT\tMISS_CT\tA1_FREQ\tBETA\tSE\t";
    text += aopt.logistic ? "Z_STAT\tP\tITER\tSTATUS\n" : "T_STAT\tP\n";
    st.header_bytes = text.size();
    auto number = [&](double v) {
        text += '\t';
        append_double(text, v, 12);
    };
    // OBS_CT MISS_CT A1_FREQ, then the fit: the part of a line that the two regressions word differently
    auto linear_tail = [&](size_t j, size_t p) {
        const stats::AssocTest r = stats::assoc_test(design, counts.data() + 4 * j, sums.data() + j * C * 4, p);
        append_u64(text, n);
        text += '\t';
        append_u64(text, counts[4 * j + 3]);
        if (r.has_freq) number(r.a1_freq);
        else text += "\tNA";
        if (r.na) {
            text += "\tNA\tNA\tNA\tNA\n";
            return;
        }
        number(r.beta);
        number(r.se);
        number(r.t);
        number(r.p);
        text += '\n';
    };
    auto logistic_tail = [&](size_t j, size_t p) {
        const uint32_t *ct = counts.data() + 4 * j;
        append_u64(text, aopt.mean_imputation ? n : n - ct[3]);
        text += '\t';
        append_u64(text, ct[3]);
        if ((uint64_t)ct[0] + ct[1] + ct[2] != 0) number(0.5 * stats::mean_dosage(ct));
        else text += "\tNA";
        const uint32_t word = status[j * P + p];
        const bool converged = (word & PGENHIP_LOGIT_CONVERGED) != 0u;
        if (converged) {
            const double b = beta[j * P + p], s = se[j * P + p], z = b / s;
            number(b);
            number(s);
            number(z);
            number(stats::wald_p(z));
            st.logit_converged++;
        } else {
            text += "\tNA\tNA\tNA\tNA";
            ++((word & PGENHIP_LOGIT_SINGULAR) ? st.logit_singular : st.logit_not_converged);
        }
        text += '\t';
        append_u64(text, word & 0xFFu);
        text += converged ? "\t.\n" : (word & PGENHIP_LOGIT_SINGULAR) ? "\tSINGULAR\n" : "\tNOT_CONVERGED\n";
    };
    for (size_t j = 0; j < V; j++) {
        const StringRecord &vr = vars[j].second;
        for (size_t p = 0; p < P; p++) {
            append_variant_columns(text, vr, a.col);
            text += vr.at(a.col[4]);   // A1: the ALT allele
            text += '\t';
            text += a.pheno_name(p);
            text += '\t';
            if (aopt.logistic) logistic_tail(j, p);
            else linear_tail(j, p);
        }
    }
    finish_text(st, text, filename, t_body);
    return st;
}

}  // namespace pgenhost
