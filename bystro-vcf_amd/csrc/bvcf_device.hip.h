// bvcf_device.hip.h — gfx950 device code of the per-line variant pipeline.
//
// Kernels, in launch order per batch:
//   k_count_eol    newline census per 1 KiB chunk              (readVcf's ReadBytes, main.go:354)
//   k_scan_groups  exclusive scan of the census, level 1
//   k_scan_top     level 2 + batch totals
//   k_scatter_eol  line start offsets from the census           ("workQueue <- buff", main.go:366)
//   k_head         16 lanes per line: tokenise the fixed columns, FILTER gate, getAlleles;
//                  emits allele records and one genotype-scan task per (line, ALT index)
//                                                                (main.go:535-545, 723-1038)
//   k_gt           one wavefront per task: the per-sample GT byte scan -> ac/an/het/hom/missing
//                  and the 2-bit class map.  THE HBM-bound kernel.   (main.go:1042-1194)
//   (from 32 768 samples up, in front of k_gt: the scans of one line split over waves --
//    k_gt_wide          one wave per (task, window of 16 384 samples) of a regular region
//    k_tabs_wide        TABs per 64 KiB share of an irregular region (a field's sample index = TABs before it)
//    k_gt_wide_general  one wave per (task, share): the general scan of the fields that start in the share
//    k_gt then adds up, or rescans a task whose regular windows met an irregular field)
//   k_finish       field-count verdict per line, scan results into the allele records
//   k_dosage       (bvcf_params.want_dosage) one wave per output allele: the int8 dosage row
//                  (k_dosage_wide: per share, for the lines k_gt_wide_general scanned)
//                                                                (main.go:1069-1178)
//   (bvcf_params.min_gq / min_dp on a file with samples, bvcf_gtfilter.hip.h: the chain above at any sample count and
//    whatever path was asked for, with
//    k_gt_filter      in place of k_gt (and of the k_gt_wide* kernels): one wave per task; the wave finds GQ / DP in the
//                     line's FORMAT column, and every lane that owns a sample field looks its values up in an LDS window
//                     of the text before it classifies the genotype -- a value below the threshold makes the sample missing
//    k_dosage_filter  in place of k_dosage: the same scan with the dosage row as output, -1 for a masked sample)
//   (bvcf_params.sample_keep on a file with samples, bvcf_gtsubset.hip.h: the same chain, again at any sample count, with
//    k_gt_subset      in place of k_gt / k_gt_filter: one wave per task walks the whole line -- n_fields is the full
//                     line's --, skips a field whose sample is not kept before anything is classified, and writes a kept
//                     sample's class at its rank among the kept samples (a {keep bits, kept before} entry per 32 samples,
//                     staged in LDS up to 32 768 samples); with a threshold it masks as k_gt_filter does
//    k_dosage_subset  in place of k_dosage / k_dosage_filter: the same task body, one dosage byte per kept sample
//    -- KernelArgs.n_samples, cmap_stride and dosage_stride are the kept samples', so every kernel behind the scan runs
//    as for a file of n_keep samples)
//
// Streaming variant for files with samples (KernelArgs.fused): the census, its scans, the scatter
// and the ALT #1 genotype scan are replaced by ONE pass over the text,
//   k_stream       one wave walks a 64 KiB tile: finds the lines that start in it, tokenises their
//                  fixed columns and scans ALT #1 straight away (the scan's loads ARE the newline
//                  search: a regular line ends where 4*ns bytes of "x|y<TAB>" end)
//   (k_stream_gen  the same for sample fields of any shape -- GT:DP:GQ ... --, bvcf_streamgen.hip.h; chosen per batch)
//   k_order        tile-local line entries -> input order and the batch's line count (a workgroup adds up the one-pass
//                  kernel's per-wave line totals and scans its own tiles' counts itself); a plain SNP line -- one-byte REF,
//                  one-byte ACGT ALT, FILTER decided -- gets its line and allele record here (bvcf_headfast.hip.h), every
//                  other line its input-ordered line_off / line_len / line_cmap / line_bits and a place in left_lines
// after which k_head (k_head_lean when blocks are in flight) takes the lines of left_lines, k_gt -- only the task slots k_head listed as holding a scan:
// deferred lines and further ALT indices of dense lines; it fills their allele records itself -- and k_finish (lines whose
// ALT #1 was deferred) run.
//
//   (bvcf_params.want_sample_stats, at the end of the chain of a file with samples: k_ss_list / k_ss_dense / k_ss_sparse
//    count, per sample, the rows whose class maps name it -- bvcf_samplestats.hip.h; k_ss_fold adds a collected batch's
//    counts to the slot's totals)
//   (bvcf_rows.hip.h holds what these and the kernels below share: which alleles[] slots are rows, reading a short list and
//    the int8 matrix-core step; bvcf_exact.h the exact-integer arithmetic)
//   (bvcf_enable_pair_stats, behind them and from the same row lists: k_pr_planes / k_pr_gemm / k_pr_sparse count, per
//    pair of samples, the rows that name both -- the bit-matrix product behind --relatedness, bvcf_pairstats.hip.h;
//    k_pr_fold adds a collected batch's tables to the ctx's totals)
//   (bvcf_enable_grm, behind them: k_grm_list lists the polymorphic rows with their quantised standard scores, k_grm_pack /
//    k_grm_gemm multiply the dense rows' int8 limbs on the matrix cores, k_grm_sparse adds the short lists' pairs -- the exact
//    integer tables behind --grm, bvcf_grm.hip.h; k_grm_fold adds a collected batch's tables to the ctx's 128-bit totals)
//   (bvcf_set_score_table, behind them: k_score_list finds every row's locus in the hash set of --score and lists the matched
//    rows with their entry, k_score_gemm multiplies the dense rows' dosages with the entries' int8 weight limbs on the matrix
//    cores -- classes expanded in registers, the tile's weights staged in LDS --, k_score_sparse adds the short lists with
//    integer atomics -- the exact fixed-point sums behind --score, bvcf_score.hip.h; k_score_fold recombines a collected
//    batch's limbs into the ctx's 128-bit totals)
//   (bvcf_set_pheno_table, behind the row index: k_assoc_list deals the rows by the form of their map, k_assoc_gemm multiplies
//    the dense rows' classes -- the map is the A operand, expanded in registers -- with the phenotypes' int8 limbs on the
//    matrix cores, reducing over the samples into one record per (row, phenotype), k_assoc_sparse does the short lists --
//    the exact integer sums behind --pheno / --assoc, bvcf_assoc.hip.h)
//   (bvcf_set_covar_table, behind those: k_assoc_cov_gemm multiplies the same classes with the int8 limbs of the covariates and
//    of their products, the column blocks dealt to workgroups as (tile, slice), k_assoc_cov_sparse does the short lists per
//    (list, family) -- the exact Gram sums behind --covar, bvcf_assoc_cov.hip.h)
//   (bvcf_set_logit_table, in their place: k_assoc_logit_gemm multiplies the classes with the int8 limbs of W C, R, R C and
//    W C C of a null model fitted on the host, an accumulator per (block, class), k_assoc_logit_sparse does the short lists per
//    (list, phenotype, family) -- the exact 128-bit sums behind --assocModel logistic, bvcf_assoc_logit.hip.h)
//   (bvcf_pca_eigen, outside every chain and without a ctx: k_pca_expand, then per step k_pca_house / k_pca_symv / k_pca_w /
//    k_pca_rank2 -- Householder tridiagonalisation of the relationship matrix in double --, and k_pca_back, the reflectors applied
//    to the eigenvectors the host found for the tridiagonal matrix -- the solver behind --pca, bvcf_pca.hip.h)
//   (bvcf_set_region_table, right behind k_finish and in front of the variant gate: k_region_gate finds every row's
//    chromosome in the hash set of --regions / --excludeRegions, binary-searches the row's span in the chromosome's merged
//    intervals and takes the unselected rows out -- bvcf_regions.hip.h)
//   (bvcf_set_variant_list, right behind k_finish and in front of the site gate: k_variant_gate walks the bytes of every
//    row's locus string "chrom:pos:ref:alt", looks it up in the hash set of --keepVariants / --excludeVariants and takes
//    the unselected rows out -- bvcf_variantlist.hip.h)
//   (bvcf_set_site_gate, right behind k_finish and in front of everything that reads a record's ac: k_site_gate takes the
//    rows out that fail --minMaf / --maxMaf / --minMac / --maxMissing / --hwe, k_site_hwe runs the exact test of the rows
//    whose support is too long for one thread, a wave per row -- bvcf_sitegate.hip.h)
//   (bvcf_enable_bed_rows, at the end of the chain of a file with samples: k_bed_count / k_bed_scan / k_bed_index give every row its
//    place in output order, k_bed_rows recodes its class map -- dense or short list -- into the unpadded row of a PLINK
//    .bed file, the rows back to back in an arena of their own -- bvcf_bedrows.hip.h)
//   (bvcf_enable_trios, behind the same row index -- built once when either is on: k_trio_count / k_trio_scan / k_trio_fill
//    give, per trio, the rows that are informative, Mendelian errors and de novo calls, and the batch's events in
//    (row, trio) order -- bvcf_mendel.hip.h)
//   (bvcf_enable_ld, behind the same row index and on the .bed arena, made once: k_ld_keys, then k_ld_pairs<false> /
//    k_ld_scan / k_ld_pairs<true> give the pairs of rows at most `window` apart whose r² reaches the threshold, as
//    events in (b, a) order -- bvcf_ld.hip.h)
//   (bvcf_params.want_name_lists, after k_finish: k_name_len / k_name_scan / k_name_write render the het / hom / missing
//    sample-name lists of every output allele as text -- main.go:612-656 -- see bvcf_names.hip.h)
//
// Sites-only input (no sample columns): k_count_eol + k_scan_* as above, then ONE pass,
//   k_sites        a wave walks a run of 8 KiB windows: text ring + TAB bit ring in LDS, line ends into a FIFO, then
//                  one lane per line for strings.Split / linePasses / getAlleles / trTv and the records
//                  (replaces k_scatter_eol + k_head + k_finish there)
// ... the default since round 3 (bvcf_sites1.hip.h), census + scans as above, then
//   k_sites2       a wave takes 7 KiB tiles behind 1 KiB of lead-in: text + TAB and terminator bitmaps in LDS, the tile's
//                  first line number from the census; one lane per line, the common lines (SNPs, lines the gate
//                  rejects) settled on fast lanes without the general getAlleles code
// ... and, kept as BVCF_SITES=3, the same body without the census (the text is read once, and it is slower):
//   k_sites1       the tile's line count published at once, the line numbers found by a decoupled look-back
//
// ... and, on request (bvcf_params.render_sites, bvcf_render.hip.h), behind k_sites2p:
//   k_render_len / k_render_scan / k_render_rows   the TSV rows of the lines the packed form settles, in input order
//
// Compressed output (bvcf_config.out_bgzf, bvcf_bgzf_deflate_device; bvcf_deflate.hip.h), on a stream of its own:
//   k_deflate      one workgroup per 65 280-byte piece of the TSV: matches, greedy parse, Huffman codes, DEFLATE bits
//   k_crc32        (bvcf_inflate.hip.h) the pieces' CRC-32
//   k_bgzf_scan / k_bgzf_pack   the members' offsets, the members packed densely for one copy to the host
//
// Everything is byte/integer work over the line bytes; no MFMA.  The genotype scans are bound by
// VALU issue at 57-70 % of the HBM peak.
// Loads are 16 B per lane, 1 KiB per wave-instruction, from the dword at or before the byte the
// record window starts at; the 0-3 byte shift is undone in registers (realign), after which every
// dword of a lane in a regular sample region ("x|y\t" per sample) is exactly one sample field.
#pragma once



#include "bvcf_common.hip.h"
#include "bvcf_rows.hip.h"
#include "bvcf_index.hip.h"
#include "bvcf_alleles.hip.h"
#include "bvcf_gtscan.hip.h"
#include "bvcf_gtfilter.hip.h"
#include "bvcf_gtsubset.hip.h"
#include "bvcf_stream.hip.h"
#include "bvcf_head.hip.h"
#include "bvcf_sites.hip.h"
#include "bvcf_sites1.hip.h"
#include "bvcf_render.hip.h"
#include "bvcf_names.hip.h"
#include "bvcf_sitegate.hip.h"
#include "bvcf_variantlist.hip.h"
#include "bvcf_regions.hip.h"
#include "bvcf_samplestats.hip.h"
#include "bvcf_pairstats.hip.h"
#include "bvcf_grm.hip.h"
#include "bvcf_pca.hip.h"
#include "bvcf_score.hip.h"
#include "bvcf_assoc.hip.h"
#include "bvcf_assoc_cov.hip.h"
#include "bvcf_assoc_logit.hip.h"
#include "bvcf_bedrows.hip.h"
#include "bvcf_mendel.hip.h"
#include "bvcf_ld.hip.h"
#include "bvcf_inflate.hip.h"
#include "bvcf_deflate.hip.h"
