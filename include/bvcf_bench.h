/*
 * bvcf_bench.h — measurement hooks of libbvcf.so.  NOT part of the drop-in ABI (include/bvcf.h): only bench.py,
 * tools/ and the size-independent property tests call these.  They replace nothing in the reference; they run the
 * same kernel chain bvcf_submit launches (launch_chain in bvcf_core.hip) over blocks that are already resident in
 * HBM, and time it with HIP events on the launch streams.
 */
#ifndef BVCF_BENCH_H
#define BVCF_BENCH_H

#include "bvcf.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Runs the kernel chain `iters` times back to back, step i on resident block i % n_blocks (each owning
 * BVCF_DEVICE_PAD bytes past its nbytes), leaving the results in device memory.  HIP events on the launch stream
 * give, per step, the time of the whole chain (chain_ms[i]) and of its dominant kernel (gt_ms[i]): k_gt on the
 * census path, k_stream / k_stream_gen on the streaming path, k_sites on the sites-only path.  counts receives {lines, alleles,
 * errs, class-map bytes, tasks} of the last step.  Returns after the last step has finished. */
int bvcf_bench_device(bvcf_ctx *ctx, const void *const *dblocks, const size_t *nbytes, int n_blocks, int iters,
                      float *chain_ms, float *gt_ms, uint64_t counts[5]);
/* the same with batch i on slot i % slots_in_use (0 = every slot of the ctx, which is what bvcf_bench_device does):
 * 1 times the chains strictly one after the other, 2 lets consecutive batches overlap as bvcf_submit would */
int bvcf_bench_device_slots(bvcf_ctx *ctx, const void *const *device_blocks, const size_t *nbytes, int n_blocks, int iters,
                            uint32_t slots_in_use, float *chain_ms, float *scan_ms, uint64_t counts[5]);

/* which kernel the streaming path will launch for the next batch: 0 = k_stream (made for the 4-byte sample grid),
 * 1 = k_stream_gen (any sample fields); the ctx picks it from the shape of the lines of the batch before
 * (-1: the ctx is not on the streaming path) */
int bvcf_bench_stream_kernel(const bvcf_ctx *ctx);

/* streaming path: how many lines of the last collected batch (bvcf_collect, bvcf_bench_device*) k_order left to k_head --
 * the ones its fast lane did not settle; -1: no batch yet, or the ctx is not on the streaming path */
long bvcf_bench_head_left(const bvcf_ctx *ctx);

/* bvcf_enable_pair_stats: the pair kernels once more over what the last bvcf_bench_device* chain of the ctx's first slot left
 * (its row lists and class maps), one after the other with HIP events around each: ms = {k_pr_planes, k_pr_gemm,
 * k_pr_sparse, k_pr_fold}.  The fold adds the batch to the ctx's totals like a collect would: for a ctx that only measures.
 * BVCF_E_ARG on a ctx without pair tables */
int bvcf_bench_pair_kernels(bvcf_ctx *ctx, float ms[4]);

/* bvcf_enable_grm: the GRM kernels once more over what the last bvcf_bench_device* chain of the ctx's first slot left (its
 * records and class maps), with HIP events around each step: ms = {k_grm_list, k_grm_pack + k_grm_gemm over every chunk,
 * k_grm_sparse, k_grm_fold}.  The fold adds the batch to the ctx's totals like a collect would: for a ctx that only measures.
 * BVCF_E_ARG on a ctx without GRM tables */
int bvcf_bench_grm_kernels(bvcf_ctx *ctx, float ms[4]);

/* bvcf_set_score_table: the score kernels once more over what the last bvcf_bench_device* chain of the ctx's first slot left
 * (its block, records and class maps), with HIP events around each step: ms = {k_score_list, k_score_gemm, k_score_sparse,
 * k_score_fold}.  The fold adds the batch to the ctx's totals like a collect would: for a ctx that only measures.
 * BVCF_E_ARG on a ctx without score tables or without a bench call before */
int bvcf_bench_score_kernels(bvcf_ctx *ctx, float ms[4]);

/* bvcf_set_pheno_table: the row index and the scan's kernels once more over what the last bvcf_bench_device* chain of the
 * ctx's first slot left (its records and class maps), with HIP events around each step: ms = {k_assoc_list, k_assoc_gemm,
 * k_assoc_sparse}.  BVCF_E_ARG on a ctx without a phenotype table or without a bench call before; BVCF_E_CAPACITY when the
 * block's rows outrun the arena (bvcf_reserve_assoc_rows) */
int bvcf_bench_assoc_kernels(bvcf_ctx *ctx, float ms[3]);
/* bvcf_set_covar_table: likewise the two kernels behind those, the row index and the scan's own kernels made once more
 * first: ms = {k_assoc_cov_gemm, k_assoc_cov_sparse}.  BVCF_E_ARG on a ctx without a covariate table or without a bench call
 * before; BVCF_E_CAPACITY when the block's rows outrun the arenas (bvcf_reserve_assoc_rows) */
int bvcf_bench_assoc_cov_kernels(bvcf_ctx *ctx, float ms[2]);
/* bvcf_set_logit_table: likewise the two kernels of the logistic model: ms = {k_assoc_logit_gemm, k_assoc_logit_sparse}.
 * BVCF_E_ARG on a ctx without a logistic table or without a bench call before; BVCF_E_CAPACITY when the block's rows outrun
 * the arenas (bvcf_reserve_assoc_rows) */
int bvcf_bench_assoc_logit_kernels(bvcf_ctx *ctx, float ms[2]);

/* The exact Hardy-Weinberg test as the site gate runs it on the device: triples = n x {het, hom, other}, p[j] the p value of
 * triple j -- by the thread-per-row recurrence or by a wave (k_site_hwe's code), chosen by the length of the support as
 * k_site_gate chooses.  Needs no ctx */
int bvcf_bench_hwe(int device, const uint32_t *triples, uint32_t n, double *p);

/* The code builder of the device compressor (step 4 of k_deflate) on given histograms, one workgroup per case, as k_deflate
 * runs it on a piece's own.  hist = n x {hll[286], hd[30], text bytes}: literal/length and distance frequencies with
 * hll[256] >= 1, at most 65 281 resp. 65 280 in sum, at most 65 280 text bytes (else BVCF_E_ARG).  lens = n x 335 bytes: the
 * 286 + 30 + 19 code lengths of the dynamic form, whatever form wins.  rle = n x 316: the run-length entries of the header
 * as sent, symbol | extra value << 8.  out = n x {kind (0 stored, 1 fixed, 2 dynamic), bits of the dynamic header, hlit,
 * hdist, hclen, entries, bytes of the dynamic form, bytes of the fixed form}.  Needs no ctx */
int bvcf_bench_deflate_codes(int device, const uint32_t *hist, uint32_t n, uint8_t *lens, uint16_t *rle, uint32_t *out);

/* bvcf_set_site_gate: the two gate kernels on their own.  The chain of the LAST block of the ctx's last bvcf_bench_device*
 * call runs once more on the first slot with the gate switched off, so that the records are as k_finish leaves them; then
 * k_site_gate and k_site_hwe run over them with HIP events around each: ms = {k_site_gate, k_site_hwe} (0 for k_site_hwe
 * when the gate has no hwe_p) -- the times of a gate that does all its work.  For this the ctx KEEPS the device pointer
 * and size of that block past the bvcf_bench_device* call: the caller must leave the block resident until it has made its
 * last bvcf_bench_gate_kernels call (or the next bvcf_bench_device* call, which replaces the pointer).  BVCF_E_ARG on a
 * ctx without a gate, or when no bvcf_bench_device* call went before */
int bvcf_bench_gate_kernels(bvcf_ctx *ctx, float ms[2]);

/* bvcf_set_variant_list: k_variant_gate on its own, as bvcf_bench_gate_kernels times the site gate -- the chain of the last
 * bench block once more on the first slot with both gates off, then the kernel over those records between two HIP events:
 * *ms.  The same rule for the block's residency.  BVCF_E_ARG on a ctx without a list, or when no bvcf_bench_device* call
 * went before */
int bvcf_bench_variant_kernel(bvcf_ctx *ctx, float *ms);
/* the alleles[] slots k_variant_gate's grid covers in one step (its threads): a batch with more rows takes a second step */
uint32_t bvcf_bench_variant_gate_stride(const bvcf_ctx *ctx);

/* bvcf_set_region_table: k_region_gate on its own, as bvcf_bench_variant_kernel times the variant gate -- the chain of the
 * last bench block once more on the first slot with all three gates off, then the kernel over those records between two
 * HIP events: *ms.  BVCF_E_ARG on a ctx without a region table, or when no bvcf_bench_device* call went before */
int bvcf_bench_region_kernel(bvcf_ctx *ctx, float *ms);
/* the alleles[] slots k_region_gate's grid covers in one step (its threads): a batch with more rows takes a second step */
uint32_t bvcf_bench_region_gate_stride(const bvcf_ctx *ctx);

/* bvcf_enable_bed_rows: the .bed kernels over the records and class maps the first slot's last bench chain left, with HIP
 * events around them: ms = {k_bed_count + k_bed_scan + k_bed_index (the row index), k_bed_rows}; out[0] = the rows, out[1] = the bytes
 * k_bed_rows wrote (rows * row_bytes).  BVCF_E_ARG on a ctx without bed rows, BVCF_E_CAPACITY when the rows outrun the arena */
int bvcf_bench_bed_kernels(bvcf_ctx *ctx, float ms[2], uint64_t out[2]);

/* bvcf_enable_trios: the trio kernels over the records and class maps the first slot's last bench chain left, with HIP
 * events around them: ms = {the row index and the two memsets, k_trio_count, k_trio_scan, k_trio_fill}; out[0] = the rows,
 * out[1] = the events.  BVCF_E_ARG on a ctx without trios, BVCF_E_CAPACITY when the events outrun the arena */
int bvcf_bench_trio_kernels(bvcf_ctx *ctx, float ms[4], uint64_t out[2]);

/* bvcf_enable_ld: the LD kernels over the records, class maps and text the first slot's last bench chain left, with HIP
 * events around them: ms = {the row index, k_bed_rows, k_ld_keys, k_ld_pairs counting, k_ld_scan, k_ld_pairs filling};
 * out[0] = the rows, out[1] = the events.  BVCF_E_ARG on a ctx without bvcf_enable_ld, BVCF_E_CAPACITY when the rows or
 * the events outrun their arena */
int bvcf_bench_ld_kernels(bvcf_ctx *ctx, float ms[6], uint64_t out[2]);

/* bvcf_pca_eigen, timed on the host between the stream waits it makes anyway: ms = {upload + k_pca_expand, the tridiagonalisation
 * (k_pca_house / k_pca_symv / k_pca_w / k_pca_rank2 over every step), the host's tridiagonal solve, upload + k_pca_back +
 * download, the whole call}.  The per-kernel split of the second entry: a kernel trace of the same call.  Needs no ctx */
int bvcf_bench_pca_eigen(int device, const float *lower, uint32_t s, uint32_t k, double *values, double *vectors, float ms[5]);

/* BVCF_POISON=XX (tests only; bvcf_devmem.h): every device and pinned buffer of a ctx created while it is set is filled
 * with the byte XX and stands between two guard zones filled with ~XX.  Reads the guards of every live buffer and returns
 * the number of buffers with a damaged guard since the last call -- live ones, and ones found damaged when they were freed;
 * each buffer counts once.  msg (cap bytes, may be NULL) receives the report of the first one: the file and line of its
 * allocation, its payload bytes, which guard, and the offset of the first damaged byte from the payload's start (negative:
 * in front of it); an empty string when there is none.  The caller has collected every batch: a kernel still running
 * would be read halfway.  0 when the mode is off.  Needs no ctx */
unsigned long bvcf_bench_guard_check(char *msg, size_t cap);
/* the buffers the mode holds alive at the moment (0 when it is off) */
size_t bvcf_bench_guarded_buffers(void);

#ifdef __cplusplus
}
#endif
#endif /* BVCF_BENCH_H */
