/*
 * scp.h - C ABI of libscp_hip.so, the MI355X-native SCP encode hot path.
 *
 * Every entry point is plain C (pointers + sizes, no torch / pybind types).  Device pointers are
 * HIP device addresses; `stream` is a hipStream_t passed as void* (NULL = default stream).
 * All functions return 0 on success or a negative SCP_E* code; nothing aborts the process.
 *
 * Each block names the reference interface it replaces (paths relative to luoao-kddi/SCP).
 * INTEGRATION.md shows the binding a reference maintainer would add for each.
 */
#ifndef SCP_H
#define SCP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SCP_API __attribute__((visibility("default")))

#define SCP_OK 0
#define SCP_EINVAL (-1)   /* bad argument (NULL, negative size, depth 0, coordinate < 0 ...) */
#define SCP_ENOMEM (-2)   /* host or device allocation failed                               */
#define SCP_ESMALL (-3)   /* caller-provided output buffer too small                        */
#define SCP_EHIP (-4)     /* a HIP runtime call failed (scp_last_hip_error() has the code)   */
#define SCP_ESTATE (-5)   /* calls made out of order on a handle                            */

#define SCP_MAX_DEPTH 21      /* 3*21 = 63 Morton bits                     */
#define SCP_MAX_SEGMENTS 62   /* trees built by one scp_geom_build call (15 / 1 when a tree has 20 / 21 levels) */

/* SCP_ABI_VERSION is what this header describes, scp_version() what the loaded library implements; a caller compares the two once
 * after loading (scp_amd/native.py does) instead of finding out through wrong numbers.  History of incompatible changes:
 *   100  rounds 1 - 2a
 *   200  WEIGHT LAYOUT: every dense entry point (scp_linear_bf16x3, scp_linear_f16x3*, scp_linear_split*, scp_mlp_split_fused and the
 *        row-chain entry points) reads its weight planes in the TILED layout of scp_tile_weight_bf16; planes straight out of
 *        scp_split_weight_bf16 / scp_split_weight_f16 (the version-100 contract) give SCP_OK and wrong products.  Pass every plane
 *        through scp_tile_weight_bf16 once, or load the library with SCP_WTILE=0 in the environment for the row-major contract;
 *        the process-wide numeric-profile setters and the debug hooks moved to scp_debug.h, scp_ctx replaces the setters.
 *   210  scp_mlp_split_fused is gone (round 4: the Swin blocks run on scp_swin_ln_linear / scp_swin_post_attn, which supersede it; two
 *        scp_linear_split calls give its bits); scp_geom_build takes float xyz through scp_geom_build_xyz as well (stage G in one
 *        launch sequence); scp_debug.h gained the launch brackets scp_prof_*.
 *   220  GELU (round 5, numeric profile ehem/5): max(y, 0) - |y| exp(-beta y^2) / P4(|y|) instead of the degree-12 erf polynomial, in every
 *        kernel that applies it; scp_swin_post_attn expects fc1 scaled by scp_gelu_prescale() and fc2 by its inverse.
 *        (additive, no new version: scp_decode_expand, scp_linear_split_f16_max, scp_row_scale_from_max, scp_octattn_attention_f16x3_vmax;
 *        round 6: scp_linear_split_hier2, scp_mlp3_rows; scp_octattn_attention_rowinv, scp_decode_expand_octattn, scp_octattn_attention_rowinv_step, scp_decode_expand_batch - existing entry points keep their bits, the EHEM model's numeric profile moved to ehem/6
 *        because models/packed.py now calls the two new ones; D2 PSNR: scp_estimate_normals_f64, scp_nn_tieset_f64;
 *        rate report: scp_rate_segments; distortion report: scp_nn_error_split_f64, scp_dist_segments_f64 - additive like the others, so
 *        SCP_ABI_VERSION and native.ABI_VERSION stay together at 220.) */
#define SCP_ABI_VERSION 220
SCP_API int scp_version(void);
SCP_API int scp_last_hip_error(void);
/* number of HIP devices visible / name of device 0 (for bench reports) */
SCP_API int scp_device_count(void);
SCP_API int scp_device_name(char *buf, int cap);

/* ------------------------------------------------------------------------------------------------
 * Numeric profile - a property of an encoder / decoder HANDLE, not of the process.
 * Two kernels offer a choice of arithmetic: the 144- / 192-feature kNN searches (dgcnn.py:10-45) run either "f16x3" (rows
 * scaled by a power of two, two f16 terms, three f16 MFMA products, fp32 accumulate: distances within ~1e-6 relative of the
 * fp32 chain; default) or the exact k-ordered fp32 MFMA chain (bit-identical distance values to PyTorch-CPU; the 3-feature
 * position search always is), and the two products inside window attention (swin_transformer.py:443-501) run either as bf16x3
 * splits on bf16 MFMA (default) or on plain fp32 MFMA.  The choice decides the last bits of the logits, i.e. the integer CDFs a
 * decoder must reproduce: an encoder and the decoder of its streams must use one profile (the stream's side-info file names it).
 * A context holds the choice; the calls of a host thread follow that thread's current context (NULL = the process default:
 * f16x3 / bf16x3 unless SCP_KNN=f32 / SCP_ATTN=f32 are set when the library is loaded).  Contexts of different threads, or
 * different contexts made current one after the other, never influence each other.
 * ---------------------------------------------------------------------------------------------- */
typedef struct scp_ctx scp_ctx;
enum { SCP_CTX_KNN_F16X3 = 1, SCP_CTX_ATTENTION_BF16X3 = 2 };
SCP_API int scp_ctx_create(scp_ctx **out);                          /* both keys 1 */
SCP_API int scp_ctx_destroy(scp_ctx *c);
SCP_API int scp_ctx_set(scp_ctx *c, int32_t key, int32_t value);    /* value 0 / 1 */
SCP_API int scp_ctx_get(const scp_ctx *c, int32_t key);             /* 0 / 1, or SCP_EINVAL */
SCP_API int scp_ctx_make_current(const scp_ctx *c);                 /* for the calling thread; NULL = process default */

/* ------------------------------------------------------------------------------------------------
 * Stage G1 - coordinate transform + quantiser
 * replaces: data_preproc/data_preprocess.py:40-68 (proc_pc) / :107-137 (mul_proc_pc),
 *           cart2spher :200-207, cart2cylin :171-177
 * ---------------------------------------------------------------------------------------------- */
enum { SCP_CART = 0, SCP_SPHER = 1, SCP_CYLIN = 2 };

typedef struct scp_quant_info {
    double bin_num;      /* round(rho_max/qs)+1 (0 for SCP_CART)            */
    double qs[3];        /* per-axis step actually used                      */
    double offset[3];    /* per-axis offset subtracted before dividing       */
    int32_t max_coord;   /* max over all points and axes of the integers     */
    int32_t min_coord;   /* min (negative => the cloud does not fit: error)  */
} scp_quant_info;

/* xyz: device float32 [n][3].  q_out: device int32 [n][3].  tr_out (optional, may be NULL): device
 * float32 [n][3] transformed coordinates (rho,phi,theta | rho,phi,z).  Synchronises `stream`
 * internally once (rho_max feeds the step sizes) and fills *info on the host. */
SCP_API int scp_quantize(const float *xyz, int64_t n, int32_t mode, double qs, double cart_offset,
                 int32_t *q_out, float *tr_out, scp_quant_info *info, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Stage G2 - octree serialisation (Morton keys -> radix sort -> per-level nodes -> occupancy)
 * replaces: data_preproc/OctreeCPP/Octree_python_lib.so `genOctreeInterface`
 *           (Octreewarpper.py:17-39,67-71), data_preproc/Octree.py:148-181 (GenOctree),
 *           :184-221 (mullevel_gen_octree), :102-137 / :224-272 (gen_K_parent_seq[_mullevel])
 * ---------------------------------------------------------------------------------------------- */
typedef struct scp_geom scp_geom; /* opaque: owns device workspace, reusable across frames */

typedef struct scp_segment {
    int64_t point_begin;  /* slice [begin, begin+count) of the q array                        */
    int64_t point_count;
    int32_t path_len;     /* rho-shell filter (Octree.py:188): 0 = keep all                   */
    int32_t path_bits;    /* path[0] is the MOST significant of the path_len low bits         */
    int32_t drop_last;    /* 1: the context tables omit the last BFS node (Octree.py:259-262) */
    int32_t reserved;
} scp_segment;

typedef struct scp_segment_info {
    int32_t depth;        /* D = ceil(log2(max+1)) over the unfiltered slice (Octree.py:58)   */
    int32_t max_coord;
    int64_t n_leaves;     /* distinct points kept                                             */
    int64_t n_nodes;      /* all tree nodes (= length of the occupancy code list)             */
    int64_t node_base;    /* first node of this segment in the concatenated tables            */
    int64_t level_count[SCP_MAX_DEPTH + 1]; /* [l] = nodes at tree level l+1                   */
} scp_segment_info;

SCP_API int scp_geom_create(scp_geom **out);
SCP_API int scp_geom_destroy(scp_geom *g);

/* q: device int32 [n][3], non-negative.  Builds every segment's tree structure (sort + counting)
 * and reports sizes; synchronises `stream` internally.  info: host array [nseg]. */
SCP_API int scp_geom_build(scp_geom *g, const int32_t *q, int64_t n, const scp_segment *segs, int32_t nseg,
                   scp_segment_info *info, void *stream);

/* The float front end and the build in ONE launch sequence (stage G1 + G2; two host read-backs instead of two per shell + three):
 * frames: nframes device arrays float32 [n_points[f]][3]; every frame is cut into nshell trees - shell s with step qs[s], the rho-shell
 * path and drop_last of shells[s] (their point_begin / point_count are ignored) - segment index = f * nshell + s.  Every point is
 * transformed once (front_transform_kernel), one kernel then quantises it per shell, applies the shell filter and writes the Morton keys
 * together with the sort's first digit histogram (front_key_kernel).  Same integers as scp_quantize, same trees as scp_geom_build.
 * qinfo / info: host arrays [nframes * nshell]; q_out (optional, may be NULL): device int32 [sum over segments of n_points][3]. */
SCP_API int scp_geom_build_xyz(scp_geom *g, const float *const *frames, const int64_t *n_points, int32_t nframes, int32_t mode,
                               const double *qs, int32_t nshell, double cart_offset, const scp_segment *shells, int32_t *q_out,
                               scp_quant_info *qinfo, scp_segment_info *info, void *stream);

/* Node tables of the last build, all segments concatenated (segment s starts at node_base[s];
 * inside a segment nodes are in BFS order = level by level, Morton order inside a level).
 * Every pointer is a device buffer of total_nodes elements and may be NULL to skip that column.
 *   occ    uint8  1..255  child-occupancy byte (= the code stream, Octreewarpper.py:71)
 *   level  uint8  1..D
 *   octant uint8  1..8
 *   parent int32  index of the parent node in the concatenated table, -1 for a root
 *   pos    int32 [total][3] node origin in leaf units (Octree.py:140-145)                      */
SCP_API int scp_geom_emit_nodes(scp_geom *g, uint8_t *occ, uint8_t *level, uint8_t *octant, int32_t *parent,
                        int32_t *pos, void *stream);

/* leaves (distinct quantised points) of segment `seg` in Morton order: device int32 [n_leaves][3] */
SCP_API int scp_geom_emit_leaves(scp_geom *g, int32_t seg, int32_t *pts, void *stream);

/* The reference's on-disk record (data_preprocess.py:74,81): int64 [rows][4][6] with channels
 * (occ 1..256, level, octant, x, y, z) for (great-grandparent, grandparent, parent, self).
 * rows = n_nodes - drop_last of segment `seg`.  out: device int64. */
SCP_API int scp_geom_krecords_i64(scp_geom *g, int32_t seg, int64_t *out, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Stage G3 - per-node context for the models
 * replaces: dataloaders/encode_dataset_ehem.py:52-105, encode_dataset_ehem_mullevel.py:47-85 (EHEM),
 *           dataloaders/encode_dataset.py:32-55 (OctAttention)
 * ---------------------------------------------------------------------------------------------- */
enum { SCP_POS_MINMAX = 0,       /* (p-min)/(max-min+1e-9), scalar min/max per level (spher/cylin) */
       SCP_POS_MINMAX_MUL = 1,   /* same, but the LAST level divides by (max-min) (mul:80)        */
       SCP_POS_POW2 = 2 };       /* p / 2^max_level (Cartesian, ehem:74)                           */

/* For segment `seg`, rows = n_nodes - drop_last:
 *   ctx    uint8 [rows][12]  (level, octant, occ-1 | 255) x (ggp, gp, p, self); levels of the LAST
 *                            tree level are clipped to lidar_level (ehem:86)
 *   pos    float32 [rows][3] normalised self position (row-major; the model API transposes)
 *   sym    uint8 [rows]      occ-1 = the symbol the arithmetic coder encodes
 *   pos_mm int64 [D][2]      (min,max) per level - DEVICE pointer, may be NULL                   */
SCP_API int scp_geom_context_ehem(scp_geom *g, int32_t seg, int32_t pos_mode, int32_t lidar_level,
                          uint8_t *ctx, float *pos, uint8_t *sym, int64_t *pos_mm, void *stream);

/* scp_geom_context_ehem for EVERY segment of the build in one launch: rows of all segments back to back (segment s starts at the sum of
 * the earlier segments' n_nodes - drop_last), pos_mm int64 [sum of depths][2], and the coded symbols in CODING ORDER (encode.py:109-136:
 * every level cut into windows of context_size rows; inside a window the even positions first, then the odd ones) - sym_coded[k] is
 * the symbol the range coder takes k-th, no coding-order index needed.  Any of pos / sym_coded / pos_mm may be NULL. */
SCP_API int scp_geom_context_ehem_all(scp_geom *g, int32_t pos_mode, int32_t lidar_level, int32_t context_size, uint8_t *ctx, float *pos,
                                      uint8_t *sym_coded, int64_t *pos_mm, void *stream);

/* OctAttention: ctx uint8 [rows][12] = (occ-1|255, level, octant) x 4; pos float32 [rows][4][3] =
 * xyz / 2^D for all four rows (no front padding - the window kernel pads on the fly). */
SCP_API int scp_geom_context_octattn(scp_geom *g, int32_t seg, uint8_t *ctx, float *pos, uint8_t *sym, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Stage M - context-model kernels (fp32).  Layouts are row-major, "tokens x channels".
 * replaces the op sequences of models/dgcnn.py:10-71, models/swin_transformer.py:443-501,625-697,
 * models/attention_model.py:58-95 (see DESIGN.md for the mapping)
 * ---------------------------------------------------------------------------------------------- */
/* k nearest neighbours in feature space, per batch item: x [B][n][C] -> idx int32 [B][n][k],
 * the k largest of  2*xi.xj - |xj|^2 - |xi|^2  (dgcnn.py:18-20), ties -> lower index. */
SCP_API int scp_knn_topk(const float *x, int32_t B, int32_t n, int32_t C, int32_t k, int32_t *idx, void *stream);

/* packed ("varlen") form for many windows in one launch: x [total_rows][C], every sequence padded to a multiple of 512 rows;
 * ctab[2c] = first row of the sequence owning 512-row chunk c, ctab[2c+1] = its real length; idx [total_rows][20] holds GLOBAL rows */
SCP_API int scp_knn_topk_packed(const float *x, const int32_t *ctab, int32_t total_rows, int32_t C, int32_t *idx, void *stream);
/* scp_knn_topk_packed with an a-priori pruning bound per row: thr0[row] = a value of (2 x.y - |x|^2 - |y|^2) that at least 20
 * candidates of the row's sequence are known to reach (e.g. the 20th best over last layer's neighbours); same result, fewer
 * list insertions.  thr0 may be NULL. */
SCP_API int scp_knn_topk_packed_bounded(const float *x, const int32_t *ctab, int32_t total_rows, int32_t C, const float *thr0,
                                int32_t *idx, void *stream);

/* edge-conv tail: out[b][i][c] = lrelu_0.2( scale[c] * (sel_j u[b][idx[b][i][j]][c] + v[b][i][c]) + shift[c] ),
 * sel = max when scale[c] >= 0 else min  (== max over j of BN(conv(edge feature)), dgcnn.py:62-71,132-134) */
SCP_API int scp_edge_gather_max(const float *u, const float *v, const int32_t *idx, const float *scale, const float *shift,
                        int32_t B, int32_t n, int32_t Cout, int32_t k, float *out, int32_t out_stride, void *stream);
/* the same with explicit row strides of u and v (floats): the two halves of one [n][2 Cout] product need no copies */
SCP_API int scp_edge_gather_max_ld(const float *u, int64_t ldu, const float *v, int64_t ldv, const int32_t *idx, const float *scale,
                           const float *shift, int32_t B, int32_t n, int32_t Cout, int32_t k, float *out, int32_t out_stride,
                           void *stream);

/* 1-D Swin window attention (window 512, 4 heads x 64): q [B][Lp][ldq], k,v [B][Lp][ldkv] already projected
 * (row strides in floats, >= 256: the operands may be column slices of a fused QKV buffer), Lp a
 * multiple of 512 (zero rows beyond L were padded AFTER LayerNorm, so their q/k/v equal the biases);
 * `shift` in {0,256}: the kernel applies the cyclic roll, the -100 mask of the last window and the
 * relative-position bias table [1023][4]; out [B][Lp][256] in un-rolled token order. */
SCP_API int scp_swin_attention(const float *q, const float *k, const float *v, const float *bias_table,
                       int32_t B, int32_t Lp, int32_t shift, int32_t ldq, int32_t ldkv, float *out, void *stream);

/* Dense layer C = epilogue(A . W^T) on bf16 MFMA with fp32-class accuracy ("bf16x3": x = hi + lo, three products, fp32
 * accumulate; replaces the nn.Linear calls of models/ehem.py / swin_transformer.py:448-452,511,559,571).
 *   scp_split_weight_bf16: W fp32 [N][K] -> bf16 planes hi/lo [Npad][Kpad] (Npad % 256 == 0, Kpad % 32 == 0, zero padded)
 *   scp_linear_bf16x3    : A fp32 [M][lda] (K % 4 == 0), the planes from above passed through scp_tile_weight_bf16 (every dense entry point
 *                          of this library streams TILED weight planes; SCP_WTILE=0: row-major), optional bias[N], residual[M][ldr];
 *                          act: 0 none, 1 LeakyReLU(0.01), 2 GELU(erf), 3 ReLU;  C fp32 [M][ldc]                        */
SCP_API int scp_split_weight_bf16(const float *W, int32_t N, int32_t K, int32_t Npad, int32_t Kpad, void *hi, void *lo, void *stream);
SCP_API int scp_linear_bf16x3(const float *A, int64_t lda, const void *Whi, const void *Wlo, int32_t Kpad, const float *bias,
                      const float *residual, int64_t ldr, float *C, int64_t ldc, int32_t M, int32_t N, int32_t K, int32_t act,
                      void *stream);

/* "f16x3" form of scp_linear_bf16x3: IEEE-half planes (22 significant bits per operand instead of 16) with one power-of-two scale
 * per row of A and per row of W (largest magnitude -> [2^13, 2^14)), undone exactly in the epilogue: the accuracy class of an
 * fp32 FMA chain at the MFMA rate of the bf16 form.  Replaces the nn.Linear calls of models/oct_attention.py:48-83 and
 * models/attention_model.py:58-125 (embeddings scaled by sqrt(600): bf16x3 misses the 1e-3 logit tolerance there).
 *   scp_split_weight_f16: W fp32 [N][K] -> scaled f16 planes hi/lo [Npad][Kpad] (Npad % 128 == 0, Kpad % 32 == 0) and
 *                         inv_scale[Npad] (1 / row scale; 1 on padding rows)
 *   scp_linear_f16x3    : as scp_linear_bf16x3; row_scale_ws = device workspace of 2 M floats (row scales of A, written here) */
SCP_API int scp_split_weight_f16(const float *W, int32_t N, int32_t K, int32_t Npad, int32_t Kpad, void *hi, void *lo,
                                 float *inv_scale, void *stream);
SCP_API int scp_linear_f16x3(const float *A, int64_t lda, const void *Whi, const void *Wlo, const float *w_inv_scale, int32_t Kpad,
                             const float *bias, const float *residual, int64_t ldr, float *C, int64_t ldc, int32_t M, int32_t N,
                             int32_t K, int32_t act, float *row_scale_ws, void *stream);
/* row scales of an activation on their own, and scp_linear_f16x3 with them given: layers that read the same rows share one pass */
SCP_API int scp_row_scale_f16(const float *A, int64_t lda, int32_t M, int32_t K, float *scale, float *inv_scale, void *stream);
SCP_API int scp_linear_f16x3_scaled(const float *A, int64_t lda, const void *Whi, const void *Wlo, const float *w_inv_scale, int32_t Kpad,
                                    const float *bias, const float *residual, int64_t ldr, float *C, int64_t ldc, int32_t M, int32_t N,
                                    int32_t K, int32_t act, const float *scale, const float *inv_scale, void *stream);

/* weight plane [Npad][Kpad] (row-major bf16, scp_split_weight_bf16) -> tiled: 1 KiB blocks ordered [16-row group][32-element k-slab],
 * each block the LDS image of one LDS-DMA instruction (row r at bytes 64 r, its 16-byte chunk q at position q ^ ((r >> 2) & 3)). */
SCP_API int scp_tile_weight_bf16(const void *plane, int32_t Npad, int32_t Kpad, void *tiled, void *stream);
/* OctAttention's dense layers on PRE-SPLIT f16 planes (oct_attention.py:48-83, attention_model.py:97-125): scp_split_rows_f16 writes, once
 * per activation tensor, what scp_linear_f16x3 converts in every tile that reads a row - the power-of-two row scale (largest magnitude
 * into [2^13, 2^14)), its inverse, and the two IEEE-half planes of the scaled row ([M][ldp], ldp >= K rounded up to 32, ldp % 8 == 0,
 * padding columns zero; K % 4 == 0, K <= 1024); scp_linear_split_f16 streams those planes by LDS-DMA (weights: scp_split_weight_f16 with
 * Npad % 256 == 0, then scp_tile_weight_bf16 per plane; act 0 none / 3 ReLU; C = act(A W^T + bias) + residual).  Bit-identical to
 * scp_linear_f16x3_scaled on the same fp32 rows. */
SCP_API int scp_split_rows_f16(const float *A, int64_t lda, int32_t M, int32_t K, void *hi, void *lo, int64_t ldp, float *scale, float *inv_scale,
                               void *stream);
/* scp_layernorm_add (below) that also writes the f16x3 operand of its output in the same pass - what scp_split_rows_f16 would make of `out` */
SCP_API int scp_layernorm_add_split_f16(const float *a, const float *b, int64_t rows, int32_t C, const float *gamma, const float *beta, float eps,
                                        float *out, void *hi, void *lo, int64_t ldp, float *scale, float *inv_scale, void *stream);
SCP_API int scp_linear_split_f16(const void *Ahi, const void *Alo, int64_t lda, const float *a_inv_scale, const void *Whi, const void *Wlo,
                                 const float *w_inv_scale, int32_t Npad, int32_t Kpad, const float *bias, const float *residual, int64_t ldr,
                                 float *C, int64_t ldc, int32_t M, int32_t N, int32_t K, int32_t act, int32_t cfg, void *stream);
/* scp_linear_split_f16 that also takes maxima of its OUTPUT in the epilogue (round 5; atomicMax on the bit patterns of |C|, the caller zeroes the
 * words before the call): row_max[M] = max |C[m][:]| (may be NULL), col_max (one word, may be NULL) = max |C[m][n]| over m < col_rows,
 * col_lo <= n < col_hi.  The power-of-two scales of the next f16x3 layer come from them without a pass over C: scp_row_scale_from_max gives what
 * scp_row_scale_f16 gives on C (attention_model.py:97-125: linear1 -> ReLU -> linear2), scp_octattn_attention_f16x3_vmax takes col_max of the
 * key | value projection for max |v|.  C is the same, bit for bit. */
SCP_API int scp_linear_split_f16_max(const void *Ahi, const void *Alo, int64_t lda, const float *a_inv_scale, const void *Whi, const void *Wlo,
                                     const float *w_inv_scale, int32_t Npad, int32_t Kpad, const float *bias, const float *residual, int64_t ldr,
                                     float *C, int64_t ldc, int32_t M, int32_t N, int32_t K, int32_t act, int32_t cfg, uint32_t *row_max,
                                     uint32_t *col_max, int32_t col_lo, int32_t col_hi, int32_t col_rows, void *stream);
SCP_API int scp_row_scale_from_max(const uint32_t *row_max, int32_t M, float *scale, float *inv_scale, void *stream);
/* The same dense layer with the ACTIVATION pre-split too: A arrives as bf16 planes hi/lo [M][lda] (lda % 8 == 0, lda >= Kpad,
 * columns K..Kpad zero) written by the producing kernel (scp_split_rows, scp_layernorm_rows_split, the attention kernels, or this
 * function's own split output), so operand tiles go global -> LDS by LDS-DMA with no conversion.  Outputs: C fp32 [M][ldc]
 * and/or planes Ohi/Olo [M][ldo] (columns N..round32(N) zero filled).  Weight planes must be padded to Npad % 256 == 0 and are
 * expected in the TILED layout of scp_tile_weight_bf16 (all scp_linear_split* entry points and the row-chain entry points; the environment
 * variable SCP_WTILE=0 switches the library to row-major [Npad][Kpad] planes, for A/B measurements).
 * cfg: 0 automatic, 1 = 256 x 256 tile, 2 = 256 x 128 tile.  Results are bit-identical to scp_linear_bf16x3 on the same values.
 *   scp_split_rows: fp32 rows -> planes, optionally gathered: out[r] = split(src[idx ? idx[r] : r]); idx == n_src -> zero row */
SCP_API int scp_linear_split(const void *Ahi, const void *Alo, int64_t lda, const void *Whi, const void *Wlo, int32_t Npad, int32_t Kpad,
                     const float *bias, const float *residual, int64_t ldr, float *C, int64_t ldc, void *Ohi, void *Olo, int64_t ldo,
                     int32_t M, int32_t N, int32_t K, int32_t act, int32_t cfg, void *stream);

/* scp_linear_split with a GATHERED residual added BEFORE the activation: out[m] = act(A[m].W^T + bias + residual[res_map[m]])
 * (res_map may be NULL = identity).  Used to evaluate a layer over concat_states (ehem.py:75-86) as one product per Swin stage. */
SCP_API int scp_linear_split_gather(const void *Ahi, const void *Alo, int64_t lda, const void *Whi, const void *Wlo, int32_t Npad, int32_t Kpad,
                            const float *bias, const float *residual, int64_t ldr, const int64_t *res_map, float *C, int64_t ldc, void *Ohi,
                            void *Olo, int64_t ldo, int32_t M, int32_t N, int32_t K, int32_t act, int32_t cfg, void *stream);
/* round 6: the two FINEST stages of such a layer in one launch (models/ehem.py:75-86,100-136: concat_states feeding ancient_mlp / prob_pred_mlp2):
 *   out[m] = act(A0[m] . W0^T + A1[parent[m]] . W1^T + bias + res[res_map[m]])  as split planes,
 * parent[m] = the stage-1 row of stage-0 row m (token t -> token t >> 1 of the same window; consecutive inside a 256-row tile), A1 with 256 columns,
 * M % 256 == 0, N % 4 == 0, weights as tiled planes.  The stage-1 product never exists in memory (it is computed per tile and stays in the
 * accumulators); summation order of an element: stage-1 k ascending, stage-0 k ascending, + bias, + residual. */
SCP_API int scp_linear_split_hier2(const void *A0hi, const void *A0lo, int64_t lda0, int32_t K0pad, const void *A1hi, const void *A1lo, int64_t lda1,
                                   int64_t M1, const void *W0hi, const void *W0lo, const void *W1hi, const void *W1lo, int32_t Npad,
                                   const int64_t *parent, const float *bias, const float *res, int64_t ldr, const int64_t *res_map, void *Ohi,
                                   void *Olo, int64_t ldo, int32_t M, int32_t N, int32_t act, void *stream);
/* scp_linear_split with SCATTERED fp32 output rows: row m goes to C row out_map[m] (negative: dropped). */
SCP_API int scp_linear_split_scatter(const void *Ahi, const void *Alo, int64_t lda, const void *Whi, const void *Wlo, int32_t Npad, int32_t Kpad,
                             const float *bias, const int64_t *out_map, float *C, int64_t ldc, int32_t M, int32_t N, int32_t K, int32_t act,
                             int32_t cfg, void *stream);
SCP_API int scp_split_rows(const float *src, int64_t ld_src, int64_t n_src, const int64_t *idx, int32_t C, void *hi, void *lo, int64_t ldo,
                   int64_t rows, void *stream);
/* producers that write the split format directly (same arithmetic as their fp32 forms, then hi = bf16(y), lo = bf16(y - hi)) */
SCP_API int scp_layernorm_rows_split(const float *x, int64_t ldx, int64_t n_src_rows, const int64_t *ia, const int64_t *ib, int32_t C,
                             const float *gamma, const float *beta, const float *valid, float eps, void *ohi, void *olo, int64_t ldo,
                             int64_t rows, void *stream);
/* out = LayerNorm(a + b) over rows of C floats (C % 4 == 0, C <= 1024; b may be NULL): the `norm(x + residual)` of
 * models/attention_model.py:117,123 (OctAttention, C = 600) in one pass. */
SCP_API int scp_layernorm_add(const float *a, const float *b, int64_t rows, int32_t C, const float *gamma, const float *beta, float eps,
                              float *out, void *stream);
SCP_API int scp_swin_attention_packed_split(const float *q, const float *k, const float *v, const float *bias_table, const int32_t *wtab,
                                    int32_t total_windows, int32_t shift, int32_t ldq, int32_t ldkv, void *ohi, void *olo, int64_t ldo,
                                    void *stream);


/* packed form: total_windows windows of 512 rows; wtab[2w] = first row of the sequence owning window w, wtab[2w+1] = its padded length */
SCP_API int scp_swin_attention_packed(const float *q, const float *k, const float *v, const float *bias_table, const int32_t *wtab,
                              int32_t total_windows, int32_t shift, int32_t ldq, int32_t ldkv, float *out, void *stream);

/* Token-wise glue of the packed forward (csrc/fused.hip):
 *   scp_layernorm_rows: out[r] = valid[r] * LayerNorm_C(row), C in {256, 512}, eps as given; row = x[r] (ia == NULL), x[ia[r]] (C 256)
 *                       or cat(x[ia[r]], x[ib[r]]) (C 512, patch merging swin_transformer.py:350-367); an index == n_src_rows is a zero row;
 *                       valid (nullable) zeroes the rows a window pads after LayerNorm (swin_transformer.py:638-641)
 *   scp_gather_rows   : out[r][0:C] = src[idx[r]][0:C] with independent row strides (concat_states ehem.py:75-86, even/odd split :113)  */
SCP_API int scp_layernorm_rows(const float *x, int64_t ldx, int64_t n_src_rows, const int64_t *ia, const int64_t *ib, int32_t C,
                       const float *gamma, const float *beta, const float *valid, float eps, float *out, int64_t ldo, int64_t rows,
                       void *stream);
SCP_API int scp_gather_rows(const float *src, int64_t lds, const int64_t *idx, int32_t C, float *out, int64_t ldo, int64_t rows, void *stream);

/* exact fp32 dense layer (k-ordered FMA chain per output, independent of the number of rows in the launch): C = act(A . W^T + bias),
 * any K / N; used for the small-K layers and for every feature that feeds a kNN search */
SCP_API int scp_linear_f32(const float *A, int64_t lda, const float *W, const float *bias, float *C, int64_t ldc, int32_t M, int32_t N, int32_t K,
                   int32_t act, void *stream);

/* OctAttention dual-stream causal attention (attention_model.py:58-95): heads of width hd,
 * q_u,k,k_u,v,v_u [B][c][H*hd] -> out, out_u [B][c][H*hd] */
SCP_API int scp_octattn_attention(const float *q_u, const float *k, const float *k_u, const float *v, const float *v_u,
                          int32_t B, int32_t c, int32_t H, int32_t hd, float *out, float *out_u, void *stream);

/* The same attention for head width 150 on f16 MFMA with fp32-class accuracy ("f16x3": every operand as two IEEE-half planes
 * with power-of-two scales - per (token, head) for q and k, one per launch for v - three MFMA products per product, fp32
 * accumulate; csrc/octattn_f16.hip).  A preparation kernel lays the planes out as LDS-DMA-ready key tiles in `workspace`
 * (device memory, 1 KiB aligned, scp_octattn_f16x3_ws_bytes(B, c, H) bytes).  q_u, k, v must be 16-byte aligned. */
SCP_API int64_t scp_octattn_f16x3_ws_bytes(int32_t B, int32_t c, int32_t H);
SCP_API int scp_octattn_attention_f16x3(const float *q_u, const float *k, const float *k_u, const float *v, const float *v_u,
                                        int64_t ldkv, int32_t B, int32_t c, int32_t H, int32_t hd, float *out, float *out_u, void *workspace,
                                        int64_t ws_bytes, void *stream);   /* ldkv: row stride (floats) of k, k_u, v, v_u - H * hd for dense
                                        rows, 1280 when they are column slices of one key | value projection (round 4); q_u, out, out_u dense */
/* the same with max |v| over the B * c rows of v GIVEN (device word: the bit pattern of a finite non-negative float, e.g. col_max of the
 * scp_linear_split_f16_max call that wrote v): no pass over v */
SCP_API int scp_octattn_attention_f16x3_vmax(const float *q_u, const float *k, const float *k_u, const float *v, const float *v_u,
                                             int64_t ldkv, int32_t B, int32_t c, int32_t H, int32_t hd, float *out, float *out_u, void *workspace,
                                             int64_t ws_bytes, const uint32_t *vmax_bits, void *stream);
/* The decodable profile's attention (octattn/1d, csrc/octattn_rowinv.hip): the same mathematics in fp32 with every output row ONE fixed
 * arithmetic sequence over rows 0..t of its own window (key tiles of 32 in ascending order from key 0, no launch-wide V scale), so a row's
 * bits do not depend on the batch, on other windows or on the query range launched.  Rows [q0, q1) of B windows; k, v: the known
 * stream's keys / values (window stride kw, row stride kr, floats; a decoder's per-layer cache); q_u, k_u, v_u, out, out_u: row r at
 * index r - qoff (strides qw / qr, uw / ur, ow / orr).  out or out_u may be NULL (that stream is skipped; with out NULL row t of k, v
 * is not read).  Head width hd <= 152. */
SCP_API int scp_octattn_attention_rowinv(const float *q_u, int64_t qw, int64_t qr, const float *k, const float *v, int64_t kw, int64_t kr,
                                         const float *k_u, const float *v_u, int64_t uw, int64_t ur, float *out, float *out_u, int64_t ow,
                                         int64_t orr, int32_t B, int32_t q0, int32_t q1, int32_t qoff, int32_t H, int32_t hd, void *stream);
/* The same attention for ONE query row per stream (the lockstep decoder's step, csrc/octattn_rowinv.hip): launch row s is the node a
 * stream is decoding; it sits at row t[slot[s]] of the window cached in slot slot[s] of k / v (`slots` windows of `rows` <= 1024 rows,
 * slot stride kw, row stride kr, floats).  t int32 [slots] and slot int32 [S] are DEVICE arrays: no stream's position is a launch
 * argument.  q_u, k_u, v_u, out, out_u: row s at s * qr / ur / orr.  Row s is bit-identical to scp_octattn_attention_rowinv with
 * q0 = t, q1 = t + 1 on that slot's cache; cache rows >= t (> t when out is wanted) and slots not listed are not read; a row whose
 * slot or t is out of range is not written.  out or out_u may be NULL. */
SCP_API int scp_octattn_attention_rowinv_step(const float *q_u, int64_t qr, const float *k, const float *v, int64_t kw, int64_t kr,
                                              int32_t slots, int32_t rows, const float *k_u, const float *v_u, int64_t ur, float *out,
                                              float *out_u, int64_t orr, const int32_t *t, const int32_t *slot, int32_t S, int32_t H,
                                              int32_t hd, void *stream);
/* The children of one decoded octree level in OctAttention's context layout (the decoder's sibling of scp_decode_expand):
 * sym / cum as there; ctx uint8 [n][12] = (occ, level, octant) x (ggp, gp, p, self) of the parents (own occupancy not read), apos int32
 * [n][4][3] the four rows' integer origins (0 for pad rows), L = the parents' level, shift = depth - L.  Child c of parent i: ctx =
 * (ctx_i[3:9], (sym_i, ctx_i[10], ctx_i[11]), (255, L + 1, digit + 1)), apos = (apos_i[1:4], origin), pos = apos / 2^depth as float. */
SCP_API int scp_decode_expand_octattn(const int64_t *sym, const int64_t *cum, const uint8_t *ctx, const int32_t *apos, int64_t n, int32_t L,
                                      int32_t shift, int32_t depth, uint8_t *cctx, int32_t *capos, float *cpos, uint8_t *occ8, void *stream);
/* OctAttention's input stage in one launch (oct_attention.py:48-66): embeddings of the four ancestors + Linear(3 -> d_pos) of their
 * positions, concatenated to D = 4 (d_occ + d_lvl + d_oct + d_pos) <= 768 channels, scaled by sqrt(D), plus the position table pe [c][D];
 * both streams (1 = "unknown": occ_enc[255] for the node's own occupancy).  ctx uint8 [n][12] = (occ, level, octant) x 4, pos fp32
 * [n][4][3], row r is position r % c of its window; levels are shifted / clipped as the reference does (level_cap 12, or 10 for obj).
 * Out: E fp32 [2][n][D] and E's f16x3 operand (planes [2 n][ldp] + row scales: what scp_split_rows_f16 makes of E). */
SCP_API int scp_octattn_embed(const uint8_t *ctx, const float *pos, int64_t n, int32_t c, const float *occ_enc, int32_t d_occ,
                              const float *level_enc, int32_t d_lvl, int32_t max_level, const float *octant_enc, int32_t d_oct,
                              const float *pos_w, const float *pos_b, int32_t d_pos, const float *pe, int32_t level_cap, float *E,
                              void *hi, void *lo, int64_t ldp, float *scale, float *inv_scale, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Stage C - softmax -> integer CDF, on device
 * replaces: torch.softmax at encode.py:126-127 + numpyAc/numpyAc.py:109-114,80-107
 * ---------------------------------------------------------------------------------------------- */
/* logits [n][nsym] (row stride `ld` floats) -> pmf [n][nsym] (may be NULL) and, if sym != NULL,
 * lohi [n]: low 16 bits = cdf[sym], high 16 bits = cdf[sym+1] (0 encodes 65536 for the top symbol).
 * cdf_full (may be NULL): uint16 [n][nsym+1] complete table (decoder / tests). */
SCP_API int scp_softmax_cdf(const float *logits, int64_t ld, int64_t n, int32_t nsym, const uint8_t *sym,
                    float *pmf, uint32_t *lohi, uint16_t *cdf_full, void *stream);
/* same, starting from a float32 PMF table (bit-exact numpyAc integer CDF) */
SCP_API int scp_pmf_cdf(const float *pmf, int64_t n, int32_t nsym, const uint8_t *sym, uint32_t *lohi,
                uint16_t *cdf_full, void *stream);

/* Rate report (csrc/rate.hip; additive, no new ABI version): where a stream's bits go.  For every row of the coding-order logits table
 *   ideal_bits = (m - x[sym] + log(sum_j exp(x[j] - m))) / ln 2   the model's cross-entropy in bits (models/ehem.py:198-210: `train_loss` is its
 *                                                                 mean per node); m = the row maximum, every term float64 from the float32 logits
 *   table_bits = 16 - log2(w), w = (hi ? hi : 65536) - lo          what the 16-bit table of scp_softmax_cdf charges for the symbol
 *   top1       = (x[sym] == m)                                     a tie with the maximum is a hit
 * summed over nseg segments of consecutive rows: seg_off int64 [nseg + 1] (DEVICE), non-decreasing, seg_off[0] = 0, seg_off[nseg] = n
 * (offsets are clamped to [0, n]; a segment may be empty).  A row with w < 1 (no table of this library has one) or with sym >= nsym is
 * counted in bad_rows, contributes 0 to both sums and is written as 0 to row_ideal / row_table; a row with a non-finite cross-entropy (the
 * symbol's logit is -inf) is counted in bad_rows and contributes 0 ideal bits, but keeps the table bits of its pair: the coder spends
 * them.  A bad row still counts in rows, and in top1 when its symbol holds the maximum.  No inf / NaN is ever written.
 * logits [n][nsym] with row stride ld >= nsym floats, 2 <= nsym <= 256.  With ld == 256 and a 16-byte aligned base the rows are read with
 * 16-byte loads, ALL 256 floats of every row: the last row's columns nsym .. 255 must then be readable memory too (as for scp_softmax_cdf;
 * the encoders' tables are [n][256]).  sym uint8 [n];
 * lohi uint32 [n] as scp_softmax_cdf writes it; out [nseg]; row_ideal / row_table float64 [n], optional (NULL).  workspace: device memory,
 * 8-byte aligned, scp_rate_workspace_bytes(n, nseg) bytes.  n == 0: SCP_OK, every segment zero (the row pointers may then be NULL).
 * Summation order is fixed - a row's sum depends on nsym alone, a segment's on its length alone - and there are no floating-point atomics:
 * a segment's sums are bit-identical from run to run, wherever the segment lies in the table, and for any ld. */
typedef struct scp_rate_seg {
    int64_t rows;
    double ideal_bits, table_bits;
    int64_t top1, bad_rows;
} scp_rate_seg;
SCP_API int64_t scp_rate_workspace_bytes(int64_t n, int32_t nseg);   /* bytes, or SCP_EINVAL for a negative argument */
SCP_API int scp_rate_segments(const float *logits, int64_t ld, int64_t n, int32_t nsym, const uint8_t *sym, const uint32_t *lohi,
                              const int64_t *seg_off, int32_t nseg, scp_rate_seg *out, double *row_ideal, double *row_table,
                              void *workspace, int64_t workspace_bytes, void *stream);

/* Per-level temperature (csrc/temper.hip; additive, no new ABI version; DESIGN.md 6, "Temperature").  A scaled logit is
 * y = fl32(beta * x), ONE float32 multiply; everything below is defined through it.
 * scp_temper_sweep: for the logits table, symbols and segments of scp_rate_segments (same layout rules, same 16-byte fast path) and a grid
 * of nt inverse temperatures betas[nt] (HOST float32, 1 <= nt <= SCP_TEMPER_MAX_NT, every one finite and > 0):
 *   seg_bits float64 [nseg][nt], seg_bad int32 [nseg][nt] (DEVICE): entry (s, j) is what scp_rate_segments writes as ideal_bits / bad_rows
 *   for segment s of the table whose every element x was replaced by fl32(betas[j] * x) - bit for bit: the same row and segment order,
 *   through the same device functions (csrc/rate_common.h).  (scp_rate_segments also counts a row whose (c_low, c_high) pair is no table
 *   entry as bad; no table scp_softmax_cdf writes has one, and the sweep takes no pairs.)  A row whose cross-entropy at beta_j is not
 *   finite, or whose symbol is outside the alphabet, adds 0 at that j and counts in seg_bad[s][j]; no inf / NaN is ever written.
 *   row_bits float64 [n][nt], optional (NULL): the rows' own bits.  workspace: device memory, 8-byte aligned,
 *   scp_temper_workspace_bytes(n, nseg, nt) bytes.  n == 0: SCP_OK, both outputs zero.  The table is read once whatever nt is; the cost is
 *   the nt * nsym float64 exponentials per row.
 * scp_temper_choose: group int32 [nseg] (DEVICE; any order; values are clamped to 0 .. ngroup - 1 on the device) assigns every segment to a
 *   group; unit is the index of the grid's 1.0f (betas[unit] == 1.0f is checked).  Per group and j the group's segments are added in
 *   segment-index order (float64, serial), and the group's choice is the j with the smallest sum - a tie goes to the index nearest unit,
 *   then to the lower index.  The group keeps unit when the best sum does not beat the unit sum by MORE than min_gain_bits (>= 0, finite:
 *   what the group's index costs as side information), when any of its segments has a bad row at any j, or when it has no rows.
 *   Outputs (DEVICE): choice int32 [ngroup], group_bits float64 [ngroup][2] (the sum at unit, the sum at the choice), seg_beta float32
 *   [nseg] (every segment's group's chosen beta).  seg_off / n as in the sweep (for the groups' row counts).
 * scp_scale_rows: out[r][c] = fl32(seg_beta[s] * in[r][c]) for c < nsym and the segment s that holds row r (seg_off int64 [nseg + 1],
 *   seg_beta float32 [nseg], both DEVICE; empty segments allowed; a row no segment holds is copied).  in / out: n rows of strides ld_in /
 *   ld_out >= nsym floats; out == in with ld_out == ld_in scales in place and then leaves columns >= nsym alone; otherwise the two must
 *   not overlap and the columns nsym .. min(ld_in, ld_out) - 1 are copied unchanged.  beta == 1.0f leaves every bit as it was (-inf and
 *   NaN payloads included: x * 1.0f is x).  With both strides 256 and 16-byte aligned bases the rows are read with 16-byte loads (all 256
 *   floats readable, as for scp_softmax_cdf).
 * All three enqueue on `stream` and wait for nothing; argument errors are found on the host before any launch (SCP_EINVAL). */
#define SCP_TEMPER_MAX_NT 32
SCP_API int64_t scp_temper_workspace_bytes(int64_t n, int32_t nseg, int32_t nt);   /* bytes, or SCP_EINVAL */
SCP_API int scp_temper_sweep(const float *logits, int64_t ld, int64_t n, int32_t nsym, const uint8_t *sym, const int64_t *seg_off,
                             int32_t nseg, const float *betas, int32_t nt, double *seg_bits, int32_t *seg_bad, double *row_bits,
                             void *workspace, int64_t workspace_bytes, void *stream);
SCP_API int scp_temper_choose(const double *seg_bits, const int32_t *seg_bad, const int64_t *seg_off, int64_t n, const int32_t *group,
                              int32_t nseg, int32_t ngroup, const float *betas, int32_t nt, int32_t unit, double min_gain_bits,
                              int32_t *choice, double *group_bits, float *seg_beta, void *stream);
SCP_API int scp_scale_rows(const float *in, int64_t ld_in, float *out, int64_t ld_out, int64_t n, int32_t nsym, const int64_t *seg_off,
                           const float *seg_beta, int32_t nseg, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Ring LOD (csrc/ringlod.hip; DESIGN.md 6, "Ring LOD"): a truncation depth per range ring, decided on integers only.
 * A TABLE is nring - 1 thresholds t_0 <= t_1 <= ... (int64, 0 .. 2^31 - 1, on axis 0 of the quantised coordinates) and nring drops
 * (uint8, 0 .. SCP_RINGLOD_MAX).  The cell of size 2^j around a position x has the origin o = (x >> j) << j per axis, the doubled radial
 * centre c2 = 2 o[0] + 2^j - 1 (int64) and the ring #{i : c2 >= 2 t_i}; it is TERMINAL iff drops[ring] >= j.
 * J(x, s) = the largest j in max(s, 1) .. max(drops) whose cell around x is terminal, 0 if there is none (drops need not be monotone).
 * scp_ringlod_cells: j[r] = J(origins[r], s_r) for n rows of int32 [n][3] (DEVICE), uint8 [n] out (DEVICE).  thresholds [ntab][nring - 1]
 *   and drops [ntab][nring] are HOST arrays (all tables of a call have nring rings; thresholds may be NULL for nring == 1), segs a HOST
 *   array of nseg disjoint row ranges.  nseg == 0: every row uses table 0 and s_r = start; level must be NULL.  nseg > 0: a row of
 *   segment k uses table segs[k].table and s_r = start, or - level (DEVICE uint8 [n], the node's octree level, root = 1) given -
 *   segs[k].depth - level[r] + 1, the size exponent of a level-L node of a tree of that depth; a row in no segment gets 0.
 *   snapped (DEVICE int32 [n][3], optional, may be `origins` itself): (x >> j[r]) << j[r] per axis.  workspace: device memory, 8-byte
 *   aligned, scp_ringlod_workspace_bytes(ntab, nseg) bytes (the tables' device image).  SCP_EINVAL - before anything is written - for
 *   NULL pointers, n < 0, nring outside 1 .. SCP_RINGLOD_MAX_RINGS, ntab / nseg above SCP_RINGLOD_MAX_TABLES, thresholds that descend,
 *   are negative or exceed 2^31 - 1, a drop above SCP_RINGLOD_MAX, overlapping or out-of-range segments, a short workspace.
 * scp_force_rows: for every row r with mask[r] != 0 (DEVICE uint8 [n]) the columns 0 .. nsym - 1 of table row r (f32, row stride ld >=
 *   nsym) become 0.0f, -1000.0f, -1000.0f, ...; other rows, and columns >= nsym, keep their bits.  scp_softmax_cdf turns such a row into
 *   (c_low, c_high) = (0, 65536 - nsym + 1) for symbol 0, and it stays one-hot under every scp_scale_rows factor of the temper grid.
 *   sym (DEVICE uint8 [n]) and mismatch (DEVICE int64 [1]) go together or are both NULL: *mismatch grows by the number of masked rows with
 *   sym[r] != 0 (integer atomic add; the caller zeroes it).  With ld == 256 and a 16-byte aligned base whole column quads are stored at once.
 * Both enqueue on `stream` and wait for nothing. */
#define SCP_RINGLOD_MAX 8
#define SCP_RINGLOD_MAX_RINGS 32
#define SCP_RINGLOD_MAX_TABLES 64
typedef struct scp_ringlod_seg {
    int64_t first, count;     /* rows first .. first + count - 1 */
    int32_t depth, table;     /* the tree's depth (read with `level` only), the rows' table */
} scp_ringlod_seg;
SCP_API int64_t scp_ringlod_workspace_bytes(int32_t ntab, int32_t nseg);   /* bytes, or SCP_EINVAL */
SCP_API int scp_ringlod_cells(const int32_t *origins, int64_t n, int32_t start, const uint8_t *level, const scp_ringlod_seg *segs, int32_t nseg,
                              const int64_t *thresholds, const uint8_t *drops, int32_t ntab, int32_t nring, uint8_t *j, int32_t *snapped,
                              void *workspace, int64_t workspace_bytes, void *stream);
SCP_API int scp_force_rows(float *table, int64_t ld, int64_t n, int32_t nsym, const uint8_t *mask, const uint8_t *sym, int64_t *mismatch,
                           void *stream);

/* ------------------------------------------------------------------------------------------------
 * Reflectance layer (csrc/attr.hip; DESIGN.md 6, "Reflectance"): an integer lifting transform on the octree of one shell.  Additive.
 * LEAVES are int32 [U][3] (DEVICE) in the order of scp_geom_emit_leaves, strictly ascending in the D-digit Morton key (digit = 4 bx +
 * 2 by + bz, axis 0 first); other orders give unspecified values, but no access leaves the buffers.  "//" is floor division.
 * scp_attr_leaf_values: q int32 [P][3], r float32 [P] (DEVICE).  v_p = clamp(floor(double(r_p) * scale + 0.5), 0, 255), 0 for a
 *   non-finite r_p; a point whose cell is a leaf adds (v_p, 1) to that leaf's (sum, cnt) with integer atomics, any other point (a
 *   coordinate outside 0 .. 2^D - 1 included) adds nothing.  Outputs (DEVICE): a uint8 [U] = (2 sum + cnt) // (2 cnt), 0 where cnt == 0;
 *   cnt int32 [U].  scale in 1 .. 2^20 (the product is then exact in a double).
 * scp_attr_forward: a uint8 [U] -> k int16 [U - 1] and ctx uint8 [U - 1] in coding order, root int32 [1], hist int32 [D][511],
 *   level_counts int64 [D + 1] (all DEVICE; hist and root are zeroed by the call).  Level-0 entries are the leaves (weight 1), the
 *   level-j entries the distinct key >> 3 j; a parent's children sit in the slots (key >> 3 (j - 1)) & 7.  A parent runs three stages,
 *   bit = 1, 2, 4: for every lo with lo & bit == 0 and lo & (bit - 1) == 0, hi = lo | bit: both present - d = v[hi] - v[lo], W = w[lo] +
 *   w[hi], m = v[lo] + (w[hi] d) // W, s = max(1, isqrt((Q Q W) // (w[lo] w[hi]))), k = sign(d) ((|d| + (s >> 1)) // s), then v[lo] = m,
 *   w[lo] = W; only hi present - it moves to lo.  Coding order: levels j = D .. 1, parents in Morton order, inside a parent stage 3, 2, 1
 *   with lo ascending; parent p of level j starts at (n_j - 1) + first[p] - p.  ctx = j - 1; hist[j - 1][z] counts z = 2 |k| - (k > 0);
 *   level_counts[j] = n_j.  U == 0 writes zeros only; U == 1 has no coefficient (k and ctx may be NULL for U <= 1).
 * scp_attr_inverse: the same tree from the weights alone, then per pair d^ = k s, v[lo] = m - (w[hi] d^) // W, v[hi] = v[lo] + d^ in int32;
 *   a uint8 [U] = the leaf values clamped to 0 .. 255.  root in 0 .. 255.
 * scp_attr_level_counts: level_counts int64 [D + 1] (DEVICE) of the same tree, nothing else (workspace of scp_attr_inverse): the
 *   coefficients of level j are (n_j - 1) .. (n_(j-1) - 2) of the coding order, so a decoder knows every context from the leaves alone.
 * scp_attr_pairs: lohi[i] = c[z_i] | c[z_i + 1] << 16 of row ctx[i] of tables uint16 [D][512] (DEVICE; entry 511 holds 65536 as 0), the
 *   pairs scp_ac_encode_lohi takes.  |k| is clamped to 255 and ctx to D - 1, so every table read is in range.
 * The workspaces are device memory, 8-byte aligned.  SCP_EINVAL before any launch for: U < 0 or U - 1 > 2^31, P outside 0 .. 2^31, D
 * outside 1 .. SCP_MAX_DEPTH, Q outside 1 .. 255, scale outside 1 .. 2^20, root outside 0 .. 255, a NULL pointer that the sizes make
 * necessary, a workspace that is NULL, misaligned or short.  Every entry enqueues on `stream` and waits for nothing. */
SCP_API int64_t scp_attr_leaf_values_workspace_bytes(int64_t U);              /* bytes, or SCP_EINVAL */
SCP_API int64_t scp_attr_forward_workspace_bytes(int64_t U, int32_t D);       /* bytes, or SCP_EINVAL */
SCP_API int64_t scp_attr_inverse_workspace_bytes(int64_t U, int32_t D);       /* bytes, or SCP_EINVAL */
SCP_API int scp_attr_leaf_values(const int32_t *q, const float *r, int64_t P, const int32_t *leaves, int64_t U, int32_t D, int32_t scale,
                                 uint8_t *a, int32_t *cnt, void *workspace, int64_t workspace_bytes, void *stream);
SCP_API int scp_attr_forward(const int32_t *leaves, const uint8_t *a, int64_t U, int32_t D, int32_t Q, int16_t *k, uint8_t *ctx, int32_t *root,
                             int32_t *hist, int64_t *level_counts, void *workspace, int64_t workspace_bytes, void *stream);
SCP_API int scp_attr_inverse(const int32_t *leaves, int64_t U, int32_t D, int32_t Q, int32_t root, const int16_t *k, uint8_t *a, void *workspace,
                             int64_t workspace_bytes, void *stream);
SCP_API int scp_attr_level_counts(const int32_t *leaves, int64_t U, int32_t D, int64_t *level_counts, void *workspace, int64_t workspace_bytes,
                                  void *stream);
SCP_API int scp_attr_pairs(const int16_t *k, const uint8_t *ctx, int64_t n, const uint16_t *tables, int32_t D, uint32_t *lohi, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Colour layer (csrc/color.hip; DESIGN.md 6, "Colour"): the RGB of an object cloud on the octree of one shell.  Additive.  LEAVES, "//",
 * the tree, the three stages of a parent, the weights, m, the step s and k are the reflectance layer's, word for word; what differs:
 * Point colour: c8 = clamp(floor(c + 0.5), 0, 255) per channel of the reader's float32 value, 0 for a non-finite one (made by the caller).
 * Leaf colour: per channel (2 sum + cnt) // (2 cnt) over the c8 of the points whose cell the leaf is, 0 where cnt == 0.
 * YCoCg-R on the leaf means, int32: Co = R - B, t = B + (Co >> 1), Cg = G - t, Y = t + (Cg >> 1); inverse t = Y - (Cg >> 1), G = Cg + t,
 *   B = t - (Co >> 1), R = B + Co (">>" arithmetic).  Y lies in 0 .. 255, Co and Cg in -255 .. 255, and the inverse is exact.
 * Lifting: the three planes Y, Co, Cg run through the same pairs with the same weights and the same step (one Q); values are int32 and
 *   are not clamped between levels; after the inverse lifting comes the inverse colour transform, and only the final R, G, B are clamped
 *   to 0 .. 255.  Q = 1 returns the leaf means exactly.  A weighted mean stays between its inputs, so |d| <= 255 for Y and <= 510 for
 *   Co / Cg: z = 2 |k| - (k > 0) <= 1020, one alphabet of 1021 symbols for the three channels.
 * scp_color_leaf_values: q int32 [P][3], rgb uint8 [P][3] (DEVICE) -> rgb_mean uint8 [U][3], ycc int16 [3][U] (planar: Y, Co, Cg), cnt
 *   int32 [U] (DEVICE); integer atomics; a point that hits no leaf (a coordinate outside 0 .. 2^D - 1 included) adds nothing.
 * scp_color_forward: ycc int16 [3][U] -> k int16 [3][U - 1] (planar, every plane in the reflectance layer's coding order), ctx uint8
 *   [U - 1] = level - 1 (shared by the planes), root int32 [3], hist int32 [3 D][1021] (row channel * D + (level - 1)), level_counts
 *   int64 [D + 1] (all DEVICE; hist and root are zeroed by the call).  U == 0 writes zeros only; k and ctx may be NULL for U <= 1.
 * scp_color_inverse: root int32 [3] (HOST: Y in 0 .. 255, Co and Cg in -255 .. 255), k as scp_color_forward writes it -> rgb uint8 [U][3].
 * scp_color_pairs: lohi uint32 [3 n] in payload order (the Y block, then Co, then Cg; n = U - 1 coefficients each): lohi[c n + i] =
 *   c[z] | c[z + 1] << 16 of row c * D + ctx[i] of tables uint16 [3 D][1022] (DEVICE; entry 1021 holds 65536 as 0).  |k| is clamped to
 *   510 and ctx to D - 1, so every table read is in range.
 * scp_attr_level_counts serves the decoder unchanged.  Workspaces, SCP_EINVAL and streams as for the reflectance layer; on unsorted or
 * repeated leaves the values are unspecified, but no access leaves the buffers: in both layers the workspace holds U entries for level 0
 * and min(U, 8^(D-j)) for level j, and every level's count is clamped to that where it is produced; level_counts returns the counts as
 * scanned, before the clamp (equal on Morton-ordered leaves). */
SCP_API int64_t scp_color_leaf_values_workspace_bytes(int64_t U);             /* bytes, or SCP_EINVAL */
SCP_API int64_t scp_color_forward_workspace_bytes(int64_t U, int32_t D);      /* bytes, or SCP_EINVAL */
SCP_API int64_t scp_color_inverse_workspace_bytes(int64_t U, int32_t D);      /* bytes, or SCP_EINVAL */
SCP_API int scp_color_leaf_values(const int32_t *q, const uint8_t *rgb, int64_t P, const int32_t *leaves, int64_t U, int32_t D, uint8_t *rgb_mean,
                                  int16_t *ycc, int32_t *cnt, void *workspace, int64_t workspace_bytes, void *stream);
SCP_API int scp_color_forward(const int32_t *leaves, const int16_t *ycc, int64_t U, int32_t D, int32_t Q, int16_t *k, uint8_t *ctx, int32_t *root,
                              int32_t *hist, int64_t *level_counts, void *workspace, int64_t workspace_bytes, void *stream);
SCP_API int scp_color_inverse(const int32_t *leaves, int64_t U, int32_t D, int32_t Q, const int32_t *root, const int16_t *k, uint8_t *rgb,
                              void *workspace, int64_t workspace_bytes, void *stream);
SCP_API int scp_color_pairs(const int16_t *k, const uint8_t *ctx, int64_t n, const uint16_t *tables, int32_t D, uint32_t *lohi, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Step sweep of the attribute layers (csrc/lift.h through csrc/attr.hip and csrc/color.hip; DESIGN.md 6, "Step sweep").  Additive.
 * The transform is open-loop: every mean m and every difference d of the two layers above is taken from exact values and does not
 * depend on Q; Q enters through s = max(1, isqrt((Q Q W) // (w[lo] w[hi]))) and k = sign(d) ((|d| + (s >> 1)) // s) alone.  For a grid
 * steps int32 [G] (HOST, 1 <= G <= SCP_SWEEP_MAX_STEPS, strictly ascending, every step in 1 .. 255) and every g (normative):
 *   hist[g]   int32 [C D][ALPHABET] = the hist of scp_attr_forward (C = 1, 511 symbols) / scp_color_forward (C = 3, 1021 symbols) at
 *             Q = steps[g], bit for bit: |k| clamped to 255 / 510, z = 2 |k| - (k > 0), row channel * D + (level - 1).
 *   sse[g]    uint64 [C_out] (C_out = 1: the reflectance; 3: R, G, B) = the sum over the leaves of (x - x^)^2, x the value that was coded
 *             (a uint8 [U]; rgb_mean uint8 [U][3]) and x^ what scp_attr_inverse / scp_color_inverse returns for the k and the root of the
 *             forward entry at Q = steps[g] - after the layer's epilogue: the clamp to 0 .. 255, for the colour behind the inverse colour
 *             transform.  Zero at Q = 1.
 *   linf[g]   uint32 [C_out] = the largest |x - x^| of the same comparison.
 * root int32 [C] and level_counts int64 [D + 1] as the forward entry writes them (neither depends on Q).  All outputs DEVICE, zeroed by
 * the call; scp_color_sweep takes ycc int16 [3][U] and rgb_mean uint8 [U][3] as scp_color_leaf_values wrote them.  Integer arithmetic
 * and integer atomics only: the outputs are functions of the inputs.  U == 0 writes zeros; U == 1 zeros, the root and the counts, and
 * launches nothing that reads a coefficient.  workspace: device memory, 8-byte aligned, scp_*_sweep_workspace_bytes(U, D, G) bytes.
 * SCP_EINVAL before any launch for the forward entries' reasons and for G outside 1 .. SCP_SWEEP_MAX_STEPS, steps NULL, a step outside
 * 1 .. 255, steps that do not strictly ascend, a NULL output.  Both enqueue on `stream` and wait for nothing; on unsorted or repeated
 * leaves the values are unspecified, but no access leaves the buffers. */
#define SCP_SWEEP_MAX_STEPS 16
SCP_API int64_t scp_attr_sweep_workspace_bytes(int64_t U, int32_t D, int32_t G);    /* bytes, or SCP_EINVAL */
SCP_API int64_t scp_color_sweep_workspace_bytes(int64_t U, int32_t D, int32_t G);   /* bytes, or SCP_EINVAL */
SCP_API int scp_attr_sweep(const int32_t *leaves, const uint8_t *a, int64_t U, int32_t D, const int32_t *steps, int32_t G, int32_t *hist,
                           uint64_t *sse, uint32_t *linf, int32_t *root, int64_t *level_counts, void *workspace, int64_t workspace_bytes,
                           void *stream);
SCP_API int scp_color_sweep(const int32_t *leaves, const int16_t *ycc, const uint8_t *rgb_mean, int64_t U, int32_t D, const int32_t *steps,
                            int32_t G, int32_t *hist, uint64_t *sse, uint32_t *linf, int32_t *root, int64_t *level_counts, void *workspace,
                            int64_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Range coder (host, serial) - replaces numpyAc/backend/numpyAc_backend.cpp
 *   encode_cdf :327-334 / encode :245-323  ->  scp_ac_encode_cdf, scp_ac_encode_lohi
 *   class decode :134-217                  ->  scp_ac_dec_*
 * ---------------------------------------------------------------------------------------------- */
SCP_API int scp_ac_encode_cdf(const uint16_t *cdf, const int16_t *sym, int64_t n, int32_t Lp, uint8_t *out, size_t cap,
                      size_t *out_len);
SCP_API int scp_ac_encode_lohi(const uint32_t *lohi, int64_t n, uint8_t *out, size_t cap, size_t *out_len);
typedef struct scp_ac_dec scp_ac_dec;
SCP_API int scp_ac_dec_new(scp_ac_dec **d, const uint8_t *stream, size_t len, int32_t Lp);
SCP_API int scp_ac_dec_next(scp_ac_dec *d, const uint16_t *cdf_row); /* returns the symbol (>= 0) */
SCP_API int scp_ac_dec_run(scp_ac_dec *d, const uint16_t *cdf, int64_t n, int16_t *out); /* n symbols, row i = CDF of symbol i */
/* n symbols, symbol i against row ctx[i] of tables [nctx][Lp] (HOST); a ctx[i] >= nctx is refused (SCP_EINVAL) before anything is decoded */
SCP_API int scp_ac_dec_run_ctx(scp_ac_dec *d, const uint16_t *tables, int32_t nctx, const uint8_t *ctx, int64_t n, int16_t *out);
SCP_API int scp_ac_dec_free(scp_ac_dec *d);

/* ------------------------------------------------------------------------------------------------
 * Chunk-parallel range coder (csrc/ac_chunks.hip, csrc/ac_chunk.h; DESIGN.md 6, "Chunked payloads").  Additive; nothing here knows what
 * the symbols are.
 * Chunked payload (normative): n symbols in payload order, a chunk size N of 64 .. 2^20 symbols, C = ceil(n / N) chunks cut by symbol
 *   index only.  The payload is C chunk lengths (little-endian uint32) followed by the C chunk byte strings.  Chunk c is BY DEFINITION the
 *   bytes scp_ac_encode_lohi returns for the pairs [c N, min(n, (c + 1) N)): a fresh coder state (low 0, high 2^32 - 1, nothing pending),
 *   the same flush, the same zero padding of the last byte.  Inside a chunk, bits behind its end read as zero, as in scp_ac_dec; a
 *   decoder reads no byte outside the chunk it decodes.
 * Version 2 of `<stream>.attr` and `<stream>.color` (version 1: the layers' sections above and DESIGN.md 6): the version byte is 2, one
 *   uint32 N follows the fixed header, the rest of the header and the per-shell records are unchanged, and a shell's payload (n = U - 1
 *   symbols for the reflectance, 3 (U - 1) for the colour: Y, Co, Cg) is a chunked payload whose "payload length" field covers the length
 *   table and the byte strings.  A reader refuses a version above 2, an N outside 64 .. 2^20, a payload too short for its ceil(n / N)
 *   lengths and a length table whose sum is not the payload length minus 4 C.
 * scp_ac_chunks_encode_lohi: lohi uint32 [n] (DEVICE, the pairs scp_ac_encode_lohi takes) -> lengths uint32 [C] (DEVICE), the C chunks
 *   packed back to back into out (DEVICE, 4-byte aligned, cap bytes), status int32 [1] (DEVICE): 0, or SCP_ESMALL when the chunks do not
 *   fit into cap - then nothing is written to out, the lengths are still complete - or when a chunk outgrew its workspace slot (pairs that
 *   no valid table produces; every store is bounds-checked).  One lane codes one chunk, then the lengths are scanned and workgroups pack.
 *   workspace: device memory, 8-byte aligned, scp_ac_chunks_workspace_bytes(n, N) bytes (C + 1 offsets and C slots of 4 ceil((18 N + 2) /
 *   32) bytes: a symbol moves at most 18 bits, derived in ac_chunk.h).  The call enqueues and returns; read lengths and status after it.
 * scp_ac_chunks_decode_ctx: bytes (DEVICE), offsets int64 [C + 1] (DEVICE, ascending, inside bytes: chunk c is bytes[offsets[c] ..
 *   offsets[c + 1])), tables uint16 [ntab][Lp] and table_of uint8 [nctx] (DEVICE), ctx uint8 [n] (DEVICE) -> sym int16 [n] (DEVICE):
 *   symbol i decoded against row table_of[ctx[i]], what scp_ac_dec_run_ctx returns on the chunk's bytes (its search, step for step, so
 *   any table decodes as on the host).  The tables and the map are held in LDS: ntab Lp 2 + nctx <= 65536 bytes.  The caller checks
 *   ctx[i] < nctx and table_of[c] < ntab; the kernel clamps both, so every table read is in range whatever they hold.
 * SCP_EINVAL before any launch for: n outside 0 .. 2^31, N outside 64 .. 2^20, cap < 0, ntab or nctx outside 1 .. 256, Lp outside 2 ..
 * 32768, tables that do not fit into LDS, a NULL or misaligned pointer that the sizes make necessary, a short workspace. */
SCP_API int64_t scp_ac_chunks_workspace_bytes(int64_t n, int64_t N);             /* bytes, or SCP_EINVAL */
SCP_API int scp_ac_chunks_encode_lohi(const uint32_t *lohi, int64_t n, int64_t N, uint32_t *lengths, uint8_t *out, int64_t cap, int32_t *status,
                                      void *workspace, int64_t workspace_bytes, void *stream);
SCP_API int scp_ac_chunks_decode_ctx(const uint8_t *bytes, const int64_t *offsets, int64_t n, int64_t N, const uint16_t *tables, int32_t ntab, int32_t Lp,
                                     const uint8_t *table_of, int32_t nctx, const uint8_t *ctx, int16_t *sym, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Legacy octree ABI - the ten symbols data_preproc/OctreeCPP/Octreewarpper.py:17-39 binds, so the
 * reference's own wrapper can load libscp_hip.so in place of Octree_python_lib.so.
 * ---------------------------------------------------------------------------------------------- */
typedef struct scp_legacy_node { uint32_t nodeid, octant, parent; uint8_t oct; uint32_t pos[3]; } scp_legacy_node;
SCP_API void *new_vector(void);
SCP_API void delete_vector(void *v);
SCP_API int vector_size(void *v);
SCP_API void *vector_get(void *v, int level);
SCP_API void vector_push_back(void *v, int i);
SCP_API void *genOctreeInterface(void *v, const double *xyz, int n);
SCP_API int Nodes_size(void *level);
SCP_API scp_legacy_node *Nodes_get(void *level, int i);
SCP_API int int_size(void *codes);
SCP_API int int_get(void *codes, int i);

/* ---- distortion metrics of the quantiser -------------------------------------------------------------
 * d2[i] = min_j |a_i - b_j|^2 in float64 (device pointers, row-major [n][3]).  Replaces the KD-tree nearest-neighbour queries
 * of data_preproc/pt.py:88-95 (distChamfer) and of the MPEG pc_error tool behind the D1 PSNR (pt.py:13-85,
 * utils/__init__.py:3-15); the host side (scp_amd/metrics.py) forms chamfer = max(mean sqrt d2_ab, mean sqrt d2_ba) and
 * PSNR = 10 log10(3 peak^2 / max(mean d2_ab, mean d2_ba)). */
SCP_API int scp_nn_sqdist_f64(const double *a, int64_t na, const double *b, int64_t nb, double *d2, void *stream);

/* D2 (point-to-plane) distortion, float64, device pointers (csrc/normals.hip; host side: scp_amd/metrics.py estimate_normals / d2_psnr).
 *
 * scp_estimate_normals_f64: what data_preproc/gene_normals.py gets from open3d (hybrid search + orientation towards the sensor).
 * The neighbours of point i are the up to max_nn (1 .. 32) nearest points with d2 <= radius^2, i itself included, ordered by d2 and
 * then by index, d2 = (dx*dx + dy*dy) + dz*dz as in scp_nn_sqdist_f64.  normals [n][3] = unit eigenvector of the smallest eigenvalue
 * of their centred covariance (cyclic Jacobi), (0,0,1) with fewer than 3 neighbours, flipped where n . (view - p) < 0; view = 3 HOST
 * doubles.  count [n] = neighbours found; idx [n][max_nn] = their indices, -1 padded (NULL: not wanted).  n <= 2^30.
 *
 * scp_nn_tieset_f64: the reductions of the MPEG pc_error tool's p2plane metric over tie sets.  p_j is a nearest neighbour of q_i iff
 * its recomputed d2 equals the minimum scp_nn_sqdist_f64 stored, bit for bit; every equal-distance neighbour counts.  Sums run in index
 * order and are divided by the count once, so the results are reproducible bit for bit.
 *   SCP_TIE_MEAN_NORMAL  dmin [np] (p against q) and nrm [np][3] belong to p; out [nq][3] = mean of nrm[j] over {j : q_i is a nearest
 *                        neighbour of p_j}, not renormalised; 0 where no p_j points at q_i.
 *   SCP_TIE_PLANE_ERROR  dmin [nq] (q against p) belongs to q, nrm [np][3] to p; out [nq] = mean over the nearest neighbours p_j of q_i
 *                        of ((q_i - p_j) . nrm[j])^2, the product summed as (dx*nx + dy*ny) + dz*nz. */
enum { SCP_TIE_MEAN_NORMAL = 0, SCP_TIE_PLANE_ERROR = 1 };
SCP_API int scp_estimate_normals_f64(const double *xyz, int64_t n, double radius, int32_t max_nn, const double *view, double *normals,
                                     int32_t *count, int32_t *idx, void *stream);
SCP_API int scp_nn_tieset_f64(int32_t mode, const double *q, int64_t nq, const double *p, int64_t np, const double *dmin, const double *nrm,
                              double *out, void *stream);

/* Distortion report (csrc/distreport.hip; additive, no new ABI version; host side: scp_amd/metrics.py distortion_report): where a frame's
 * error goes - per range ring and per caller-given group (the encoder: per rho shell), split along the sensor's spherical axes.
 * A = the query cloud [na][3], B = the searched cloud [nb][3], float64 DEVICE pointers, finite coordinates, 1 .. 2^30 points each;
 * view = the sensor position, 3 HOST doubles.
 *
 * scp_nn_error_split_f64, per query i:
 *   neighbour  d2(i,j) = (dx*dx + dy*dy) + dz*dz, dx = a_i.x - b_j.x ..., the arithmetic and rounding of scp_nn_sqdist_f64;
 *              d2_out[i] = min_j d2(i,j) and idx_out[i] = j*(i) = the LOWEST j whose d2(i,j) equals that minimum bit for bit.  Both come
 *              from integer atomicMin reductions, so neither depends on how the launch splits B or on the order tiles are visited in.
 *   split      e = b_j* - a_i.  With (x,y,z) = a_i - view, s2 = x*x + y*y, s = sqrt(s2), rho2 = s2 + z*z, rho = sqrt(rho2):
 *              r^ = (x,y,z)/rho, phi^ = (-y,x,0)/s, theta^ = (xz, yz, -s2)/(rho s) (growing polar angle arccos(z/rho));
 *              comp_out[i] = (e.r^, e.phi^, e.theta^), accurate to a few ulp of |e|.  s == 0 (on the sensor's axis, or at the sensor):
 *              no frame - an AXIS point: comp_out[i] = 0 and SCP_DIST_FLAG_AXIS in flag_out[i].
 *   bin        edges_sq = n_rings HOST doubles, the SQUARES of the ring edges 0 = E_0 < E_1 < ... (finite, strictly increasing; the last
 *              ring is open-ended; 1 <= n_rings <= SCP_DIST_MAX_RINGS).  ring(i) = the largest r with rho2 >= edges_sq[r]: decided on
 *              rho2, no sqrt takes part, a point exactly on an edge belongs to the upper ring.  group int32 [na] (DEVICE; NULL: all 0),
 *              0 <= group[i] < n_groups; bin_out[i] = group[i] * n_rings + ring(i); n_groups * n_rings <= SCP_DIST_MAX_BINS.
 *              A group value outside [0, n_groups) is CLAMPED in the kernel and the row flagged SCP_DIST_FLAG_GROUP_CLAMPED, so no bin is
 *              ever out of range (scp_amd/native.py checks the range before the launch and refuses).
 *   A query no pair of which reproduces the minimum (only non-finite coordinates do that) gets idx -1, d2 0, components 0 and
 *   SCP_DIST_FLAG_NO_NEIGHBOUR; nothing is read through its index.
 * Every argument is checked before any launch: a NULL pointer (group excepted), na / nb outside 1 .. 2^30, n_groups < 1, n_rings outside
 * 1 .. SCP_DIST_MAX_RINGS, edges that do not start at 0 or do not strictly increase, more than SCP_DIST_MAX_BINS bins or a non-finite
 * view return SCP_EINVAL.
 *
 * scp_dist_segments_f64: one scp_dist_seg per bin from the per-query values above.  The rows of bin k are order[seg_off[k]] ..
 * order[seg_off[k+1] - 1] (order int64 [n], DEVICE: a STABLE sort of the bins, so that a bin's rows come in index order; NULL: the rows
 * lie in bin order already; seg_off int64 [n_bins + 1], DEVICE, non-decreasing; offsets are clamped to [0, n] and an order entry outside
 * [0, n) is skipped).  Summation order is part of the contract: thread t of the bin's one workgroup adds rows t, t + 1024, .. of the bin
 * in that order, then a fixed binary tree runs over the 1024 partial sums - a bin's sums are a function of that bin's rows in index
 * order and of nothing else (not of the other bins, of n_bins or of the launch), the same bits in every run; no floating-point atomics.
 *   rows, axis_rows   all rows of the bin / its axis points (which count in rows, sum_sq, max_sq and hist and add nothing to the other sums)
 *   sum_sq = sum d2, sum_r2 = sum e_r^2, sum_phi2 = sum e_phi^2, sum_theta2 = sum e_theta^2, sum_r = sum e_r;  max_sq = max d2 (0: empty bin)
 *   hist[0] = rows with d2 == 0; hist[k] = rows with k == clamp(floor(log2 d2) + 41, 1, 63), read from the exponent bits: bucket k holds
 *   2^(k-41) <= d2 < 2^(k-40), both tails absorbed.
 * n outside 1 .. 2^30, n_bins outside 1 .. SCP_DIST_MAX_BINS or a NULL pointer (order excepted): SCP_EINVAL, nothing launched. */
#define SCP_DIST_MAX_RINGS 64
#define SCP_DIST_MAX_BINS 4096
#define SCP_DIST_MAX_POINTS (1ll << 30)
enum { SCP_DIST_FLAG_AXIS = 1, SCP_DIST_FLAG_GROUP_CLAMPED = 2, SCP_DIST_FLAG_NO_NEIGHBOUR = 4 };
typedef struct scp_dist_seg {
    int64_t rows, axis_rows;
    double sum_sq, sum_r2, sum_phi2, sum_theta2, sum_r, max_sq;
    int64_t hist[64];
} scp_dist_seg;
SCP_API int scp_nn_error_split_f64(const double *a, int64_t na, const double *b, int64_t nb, const double *view, const double *edges_sq,
                                   int32_t n_rings, const int32_t *group /* NULL ok */, int32_t n_groups, int32_t *idx_out, double *d2_out,
                                   double *comp_out /* [na][3] */, int32_t *bin_out, uint8_t *flag_out, void *stream);
SCP_API int scp_dist_segments_f64(const double *d2, const double *comp, const uint8_t *flag, const int64_t *order /* NULL ok */, int64_t n,
                                  const int64_t *seg_off, int32_t n_bins, scp_dist_seg *out, void *stream);

/* Rate per range ring (csrc/ringrate.hip; additive, no new ABI version; host side: scp_amd/metrics.py ring_rate_dict, FrameEncoder.ring_rate):
 * every leaf's share of its ancestors' bits, summed over the bins of the distortion report - so that "what does the 40 - 60 m ring cost,
 * and what error does it buy" has an answer.  Definition, for one tree (one segment of a scp_geom build; nodes in BFS order, depth D):
 *   leaves(i) = popcount(occ_i) for a node of level D, the sum over the node's children otherwise (the level-D total is n_leaves);
 *   bits(i)   = what the caller says node i cost, two columns (ideal, table) - the encoder: row_ideal / row_table of the node's coded row
 *               (scp_rate_segments), 0 for the node a drop_last segment leaves uncoded;
 *   share(i)  = bits(i) / (double)leaves(i), one IEEE float64 division;
 *   cost(p)   = ((share(a_1) + share(a_2)) + ..) + share(a_D), a_l = the ancestor of leaf p at level l: root first, float64, no fused
 *               operation - a numpy loop reproduces it bit for bit;
 *   leaf p    = in the order of scp_geom_emit_leaves: level-D node j owns the popcount(occ_j) consecutive leaves that start at the
 *               exclusive prefix sum of the popcounts of the level-D nodes before it.
 * The sum of cost over the leaves equals the sum of bits over the nodes up to rounding (every node's bits are handed out in leaves(i)
 * equal parts).
 *
 * scp_rate_leaf_share: occ / level uint8, parent int32 (index into the concatenated table, -1 for a root), bits_ideal / bits_table
 * float64, all DEVICE [total_nodes] - the columns of scp_geom_emit_nodes for all segments of a build; segs = nseg HOST rows of four
 * int64 (node_base, n_nodes, depth, leaf_base) that tile the node table and the leaf table in this order (segment s owns the leaves
 * leaf_base[s] .. leaf_base[s + 1] - 1, the last one up to total_leaves - 1; at least one node and one leaf each).  Outputs (DEVICE):
 * leaves int64 [total_nodes]; cost_ideal, cost_table float64 [total_leaves], segment-major, Morton order inside a segment.  workspace:
 * device memory, 8-byte aligned, scp_rate_leaf_share_workspace_bytes(total_nodes, nseg) bytes.
 * Every argument is checked on the host before any launch: a NULL pointer, total_nodes / total_leaves outside 1 .. 2^30, nseg outside
 * 1 .. SCP_MAX_SEGMENTS, a depth outside 1 .. SCP_MAX_DEPTH, a segment table that does not tile both tables, a workspace too small or
 * misaligned: SCP_EINVAL.  The node table itself is then checked by a validation launch before any index in it is followed: per
 * segment the first node is the only node of level 1 and has parent -1; levels lie in 1 .. depth and never fall along the table; a
 * parent lies inside the segment, in front of its child, one level up; parents never fall along a level; no occ is 0; the level-D
 * popcounts add up to the segment's leaf count.  A table that breaks a rule returns SCP_EINVAL (one small read-back: the call
 * synchronises `stream` once); nothing is written through an index taken from it.
 * Order: leaves by integer atomics, one launch per level bottom-up; cost one launch per level top-down, a node adding its share to its
 * parent's finished sum.  All segments share the launches, whose number (2 * deepest tree + 1) depends on the depths alone.
 *
 * scp_ring_bins_f64: the bin of scp_nn_error_split_f64's bin_out for a cloud of its own - xyz float64 DEVICE [n][3], view / edges_sq /
 * n_rings / group / n_groups exactly as there, the same expressions on the same operands (rho2 = (x*x + y*y) + z*z of xyz - view; ring =
 * the largest r with rho2 >= edges_sq[r]; bin = group * n_rings + ring): integer for integer the same bins.  flag_out uint8 [n]
 * (optional, NULL): SCP_DIST_FLAG_GROUP_CLAMPED where a group outside [0, n_groups) was clamped.  Argument checks as there.
 *
 * scp_share_segments_f64: one scp_share_seg per bin; rows, order, seg_off, clamping and the SUMMATION CONTRACT exactly as
 * scp_dist_segments_f64 (thread t adds rows t, t + 1024, .. of the bin in that order, a fixed binary tree over the 1024 partial sums; no
 * floating-point atomics; a bin's record depends on that bin's rows in index order and on nothing else).
 *   leaves = rows of the bin; ideal_bits = sum cost_ideal; table_bits = sum cost_table; max_ideal_bits = max cost_ideal (0: empty bin)
 * n outside 1 .. 2^30, n_bins outside 1 .. SCP_DIST_MAX_BINS or a NULL pointer (order excepted): SCP_EINVAL, nothing launched. */
#define SCP_SHARE_MAX_NODES (1ll << 30)
typedef struct scp_share_seg {
    int64_t leaves;
    double ideal_bits, table_bits, max_ideal_bits;
} scp_share_seg;
SCP_API int64_t scp_rate_leaf_share_workspace_bytes(int64_t total_nodes, int32_t nseg);   /* bytes, or SCP_EINVAL */
SCP_API int scp_rate_leaf_share(const uint8_t *occ, const uint8_t *level, const int32_t *parent, int64_t total_nodes, const double *bits_ideal,
                                const double *bits_table, const int64_t *segs /* HOST [nseg][4] */, int32_t nseg, int64_t total_leaves,
                                int64_t *leaves, double *cost_ideal, double *cost_table, void *workspace, int64_t workspace_bytes, void *stream);
SCP_API int scp_ring_bins_f64(const double *xyz, int64_t n, const double *view, const double *edges_sq, int32_t n_rings,
                              const int32_t *group /* NULL ok */, int32_t n_groups, int32_t *bin_out, uint8_t *flag_out /* NULL ok */, void *stream);
SCP_API int scp_share_segments_f64(const double *cost_ideal, const double *cost_table, const int64_t *order /* NULL ok */, int64_t n,
                                   const int64_t *seg_off, int32_t n_bins, scp_share_seg *out, void *stream);

/* Depth report (csrc/ringrate.hip; additive, no new ABI version; host side: scp_amd/metrics.py depth_dict, FrameEncoder.depth_report):
 * what the first D - k levels of a tree cost, per leaf and per bin - an octree stream is progressive, its levels 1 .. D - k describe the
 * cloud at cell size 2^k.  With leaves(i), share(i), the ancestors a_l and the leaf order of the rate per ring above:
 *   cost_k(p) = ((share(a_1) + share(a_2)) + ..) + share(a_{D-k})   for 0 <= k < D: the operations of cost(p), the chain cut short;
 *   cost_k(p) = +0.0                                                for k >= D.
 * cost_0 is scp_rate_leaf_share's cost bit for bit; float64, no fused operation, no floating-point atomics.
 *
 * scp_rate_depth_share: the arguments of scp_rate_leaf_share plus max_drop (0 .. SCP_MAX_DEPTH).  Outputs (DEVICE): leaves int64
 * [total_nodes]; cost_ideal, cost_table float64 [(max_drop + 1) * total_leaves], plane k (= cost_k of every leaf, in the leaf order of
 * scp_rate_leaf_share) at offset k * total_leaves.  workspace: scp_rate_depth_share_workspace_bytes(total_nodes, nseg) bytes, 8-byte
 * aligned device memory.  The host checks and the validation launch of scp_rate_leaf_share apply unchanged, and max_drop outside its
 * range is refused with them: SCP_EINVAL, nothing written to an output (the call synchronises `stream` once).
 * Order: leaves, the per-node sums and plane 0 by the launches of scp_rate_leaf_share; then, for max_drop >= 1, one launch in which every
 * level-D node climbs up to max_drop parents and writes planes 1 .. max_drop of the leaves it owns.  All segments share the launches,
 * whose number (2 * deepest tree + 2; + 1 for max_drop = 0) depends on the depths alone - not on node or segment counts.
 *
 * scp_share_segments_depth_f64: scp_share_segments_f64 on n_depths planes in one launch (depth on the second grid axis): plane d of
 * cost_ideal / cost_table starts at d * plane_stride (>= n); order, seg_off, n, clamping and the SUMMATION CONTRACT exactly as there, the
 * same for every plane.  out: scp_share_seg [n_depths][n_bins]; record [0][b] equals what scp_share_segments_f64 returns on plane 0,
 * field for field.  n_depths outside 1 .. SCP_MAX_DEPTH + 1, plane_stride < n or > 2^30, or an argument scp_share_segments_f64
 * refuses: SCP_EINVAL, nothing launched. */
SCP_API int64_t scp_rate_depth_share_workspace_bytes(int64_t total_nodes, int32_t nseg);   /* bytes, or SCP_EINVAL */
SCP_API int scp_rate_depth_share(const uint8_t *occ, const uint8_t *level, const int32_t *parent, int64_t total_nodes, const double *bits_ideal,
                                 const double *bits_table, const int64_t *segs /* HOST [nseg][4] */, int32_t nseg, int64_t total_leaves,
                                 int32_t max_drop, int64_t *leaves, double *cost_ideal, double *cost_table, void *workspace,
                                 int64_t workspace_bytes, void *stream);
SCP_API int scp_share_segments_depth_f64(const double *cost_ideal, const double *cost_table, const int64_t *order /* NULL ok */, int64_t n,
                                         const int64_t *seg_off, int32_t n_bins, int32_t n_depths, int64_t plane_stride, scp_share_seg *out,
                                         void *stream);

/* Input stage of the packed EHEM forward: embeddings of dgcnn.py:121-128 fused with the packed layout's input gather.
 * ctx u8 [T][12] = 4 x (level, octant, occ) (scp_geom_context_ehem), pos f32 [T][3], inmap i64 [rows] (== n_tokens: pad token);
 * tables occ_enc [256][16], level_enc [*][4], octant_enc [*][4]; out x f32 [rows][80], pos_out f32 [rows][3], occ_self i64 [rows]. */
SCP_API int scp_embed_gather(const uint8_t *ctx, const float *pos, const int64_t *inmap, int64_t n_tokens, const float *occ_enc,
                     const float *level_enc, const float *octant_enc, float *x, float *pos_out, int64_t *occ_self, int64_t rows,
                     void *stream);

/* ---- index maps of the packed ("varlen") EHEM forward ------------------------------------------------------------------
 * lengths[W] (host): the window lengths of one packed chunk (encode.py:109-136 cuts every level into windows of <= 8192 nodes).
 * scp_packed_plan_sizes: rows of the 11 layouts (self stages 0..4, cross stages 0..3, even outputs, odd outputs; every window
 * padded to x512 rows per Swin stage).  scp_packed_plan: writes all 56 maps in one launch; outs[] = device buffers in this order:
 *   inmap i64[rows0]; a1map, a2map i64[rowsX0]; even_rows i64[E]; odd_rows i64[O]; even_dst i64[E]; odd_dst i64[O];
 *   self merge (even, odd) i64[rows s+1] for s = 0..3; cross merge (even, odd) for s = 0..2; self concat i64[rows0] for s = 1..4;
 *   cross concat i64[rowsX0] for s = 1..3; window tables i32[rows/512][2] (base, padded length) of the 9 stage layouts;
 *   kNN table i32[rows0/512][2] (base, real length); valid f32[rows] of the 9 stage layouts; parent-row maps i64[rows s] (stage s
 *   token t -> stage s+1 token t >> 1) for self s = 0..3 and cross s = 0..2; coded positions i64[rowsX0] of the even / odd token
 *   of every cross-stage-0 row (-1 for padding rows).
 * Replaces the per-window Python bookkeeping of models/ehem.py:88-136 / swin_transformer.py:350-367,638-641 in the packed forward;
 * tables_dev: int64 scratch of 36 * W entries. */
SCP_API int scp_packed_plan_sizes(const int64_t *lengths, int32_t W, int64_t *rows_out);
SCP_API int scp_packed_plan(const int64_t *lengths, int32_t W, int64_t *tables_dev, void *const *outs, int32_t n_outs, void *stream);

/* ---- decoder: the children of one decoded octree level + the model inputs of the level they form, one launch ------------------
 * replaces: decode_ehem_mullevel.py:100-130 (decode_ehem.py likewise): child occupancy bits -> (parent, digit) pairs in breadth-first
 * order, the ancestor window shifted by one, cal_pos_ary (:41-53), the next level's context rows and normalised positions.
 *   sym i64[n]: decoded symbols of the parents (occupancy - 1; -1 = unknown: no children); cum i64[n]: INCLUSIVE scan of popcount(sym + 1);
 *   pos i32[n][3] node origins; anc u8[n][9] = (level, octant, symbol) of (ggp, gp, p), 255 = pad; octant u8[n]; L = the parents' level;
 *   shift = depth - L.  Outputs for the m = cum[n - 1] children: cpos i32[m][3], canc u8[m][9], coct u8[m], cctx u8[m][12] (ancestor
 *   levels clamped to lv_clamp, own entry (lv_next, octant, 255)), cposn f32[m][3] = polar ? (pos - mn) / den : pos / den (double
 *   arithmetic, rounded once), occ8 u8[n] = the parents' occupancy codes. */
SCP_API int scp_decode_expand(const int64_t *sym, const int64_t *cum, const int32_t *pos, const uint8_t *anc, const uint8_t *octant, int64_t n,
                              int32_t L, int32_t shift, int32_t lv_next, int32_t lv_clamp, int32_t polar, double mn, double den, int32_t *cpos,
                              uint8_t *canc, uint8_t *coct, uint8_t *cctx, float *cposn, uint8_t *occ8, void *stream);

/* The same for the decoded levels of S (1 .. 64) streams at once, ONE launch (the lockstep decoder, scp_amd/decoder.py: EhemBatchDecoder).
 * The parents of the streams ("segments") lie back to back in sym / pos / anc / octant [n]; cum is the inclusive scan of popcount(sym + 1)
 * over the WHOLE array.  seg[S] (host memory): per segment its first parent row and parent count (first[0] = 0, contiguous, count >= 1),
 * scp_decode_expand's scalars (L, shift, lv_next, lv_clamp, polar, mn, den: the streams differ in depth, lidar level and coordinate
 * system), cfirst = its first child row (= the scan's value before the segment; the children of all segments back to back, M in all)
 * and coded <= its child count = the children that get model-input rows.  Child c of segment s: state row cfirst[s] + c of cpos / canc /
 * coct [M]; for c < coded[s], input row wbase[(c / cs) * S + s] + c % cs of cctx u8[T][12] / cposn f32[T][3] - wbase i64[K][S] (host
 * memory) = the first row of window k of segment s in the caller's window order (-1: no such window).  Per-element arithmetic and bits
 * are scp_decode_expand's.  table_dev: the caller's DEVICE copy of both tables, uploaded on `stream` before the call - seg[S] at byte 0,
 * wbase[K][S] at byte 64 * sizeof(scp_expand_seg); the entry copies nothing and waits for nothing.  Everything is checked on the
 * host (on the host tables) before any launch (SCP_EINVAL): pointers, S, cs, K, the level and shift ranges of scp_decode_expand, the segment table's
 * consistency with n and M, and that every window a coded child lands in lies inside [0, T).  Additive: no new ABI version. */
typedef struct scp_expand_seg {
    int64_t first, count, cfirst, coded;
    int32_t L, shift, lv_next, lv_clamp, polar, reserved;
    double mn, den;
} scp_expand_seg;
SCP_API int scp_decode_expand_batch(const int64_t *sym, const int64_t *cum, const int32_t *pos, const uint8_t *anc, const uint8_t *octant,
                                    int64_t n, const scp_expand_seg *seg, int32_t S, int32_t cs, const int64_t *wbase, int32_t K, int64_t M,
                                    int64_t T, void *table_dev, int32_t *cpos, uint8_t *canc, uint8_t *coct, uint8_t *cctx, float *cposn,
                                    uint8_t *occ8, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Swin blocks on the row-chain kernels (csrc/rowchain.hip): a workgroup keeps 128 token rows in registers as the B operand of
 * every product, weights stream through LDS, and the accumulator of one product is the B fragment of the next.
 * replaces: models/swin_transformer.py:654-706 (SwinLayer.forward) around the attention kernel -
 *   scp_swin_ln_linear : layernorm_before + query|key|value (:443-501,654-660), or layernorm(query) + query of a cross layer:
 *                        out[m] = valid[m] * n(x[m]) . W'^T + bias + valid[m] * wbeta, n = the row normalised WITHOUT affine;
 *                        the caller folds the LayerNorm affine into the weight: W' = W diag(gamma), wbeta = W beta.  valid (may be
 *                        NULL) zeroes the rows a window pads AFTER LayerNorm (:638-641): they come out as the bias alone.
 *                        x fp32 [M][ldx] (256 channels); W' as scp_split_weight_bf16 + scp_tile_weight_bf16 planes [Npad][256];
 *                        N % 128 == 0, N <= 1024; out fp32 [M][ldo].
 *   scp_swin_post_attn : attention.output.dense + residual, layernorm_after, intermediate.dense + GELU, output.dense + residual
 *                        (:503-571,662-706) in ONE launch: x2 = x1 + fc2(GELU(fc1(LN(x1)))), x1 = x + proj(o).  o: the attention
 *                        output as bf16 hi/lo planes [M][ldo_in]; x fp32 [M][ldx]; out fp32 [M][ldc] (may be x).  W: ONE buffer of
 *                        scp_swin_post_attn_weight_bytes() bytes = tiled planes proj hi | fc1 hi | fc2 hi | proj lo | fc1 lo | fc2 lo,
 *                        proj [256][256], fc1 = (W1 diag(gamma))[:, P] [1024][256], fc2 = W2[:, P] [256][1024], P = inside every
 *                        16 columns, columns 4-7 and 8-11 change places (the order in which an MFMA accumulator holds a row's
 *                        channels); b1 = fc1 bias + W1 beta.  Since version 220 the kernel evaluates GELU in the variable s y
 *                        (s = scp_gelu_prescale()): the caller multiplies fc1 (weight and b1) by s and divides fc2's weight by s.
 * Results are per row: independent of M, of the row's position and of what else is in the launch.
 * ----------------------------------------------------------------------------------------------  * tile_list (device int32 [n_tiles], ascending; may be NULL = every tile): the 128-row tiles to process.  The packed forward passes the
 * tiles that hold at least one real row: tiles of nothing but window padding (4.7 % of a level-16 multi-level frame) keep their old
 * contents - run it in place (out == x) so that these stay finite. */
SCP_API int scp_swin_ln_linear(const float *x, int64_t ldx, const float *valid, const void *Whi, const void *Wlo, const float *bias,
                               const float *wbeta, float eps, float *out, int64_t ldo, int32_t M, int32_t N, void *stream);
SCP_API int scp_swin_post_attn(const void *Ohi, const void *Olo, int64_t ldo_in, const float *x, int64_t ldx, const void *W, const float *bp,
                               const float *b1, const float *b2, float eps, float *out, int64_t ldc, int32_t M, const int32_t *tile_list,
                               int32_t n_tiles, void *stream);
SCP_API int64_t scp_swin_post_attn_weight_bytes(void);
SCP_API double scp_gelu_prescale(void);

/* SwinPatchMerging (swin_transformer.py:350-384) in one launch: out[m] = LayerNorm(cat(x[ia[m]], x[ib[m]])) . W^T for M merged rows (the
 * reduction has no bias).  x: fp32 [n_src][ldx] (256 channels; an index equal to n_src stands for a row of zeros - the pad of an odd
 * window); W: a buffer of scp_swin_post_attn_weight_bytes() bytes holding the tiled planes (scp_split_weight_bf16 + scp_tile_weight_bf16) of
 * (W diag(gamma))[:, 0:256] at byte 0 and of (W diag(gamma))[:, 256:512] at byte 131072, their lo planes at the same offsets behind the
 * first half of the buffer; wbeta = W beta [256]; out fp32 [M][ldo]. */
SCP_API int scp_swin_merge(const float *x, int64_t ldx, int64_t n_src, const int64_t *ia, const int64_t *ib, const void *W, const float *wbeta,
                           float eps, float *out, int64_t ldo, int32_t M, void *stream);

/* The two edge MLPs of the geometry feature generator (dgcnn.py:121-151: edge_mlp1 448 -> 256 -> 256 -> 256 on cat(pos1, pos2, pos3), edge_mlp2
 * 512 -> 256 -> 256 -> 128 on cat(pos3, edge_mlp1(...)), LeakyReLU(0.01) between the layers) for M points in one launch: six dense layers
 * chained through the MFMA accumulators.  pos1 / pos2 / pos3: fp32 [M][64 | 128 | 256] (row strides ld1 / ld2 / ld3); W: a buffer of
 * scp_swin_post_attn_weight_bytes() bytes with eight tiled [256][256] matrices (hi planes at m * 131072 bytes, lo planes at the same
 * offsets behind the first half of the buffer): 0 / 1 = edge_mlp1 layer 1, input columns [0, 256) / [256, 448) + 64 zero columns;
 * 2, 3 = its layers 2, 3; 4 / 5 = edge_mlp2 layer 1, input columns [256, 512) / [0, 256); 6, 7 = its layers 2, 3 (7: 128 rows); the
 * input columns of matrices 2, 3, 4, 6, 7 in accumulator order (inside every group of 16: columns 4 - 7 and 8 - 11 exchanged);
 * bias: the six bias vectors back to back (1408 floats); out: fp32 [M][ldo], 128 columns written. */
SCP_API int scp_geo_edge_mlps(const float *pos1, int64_t ld1, const float *pos2, int64_t ld2, const float *pos3, int64_t ld3, const void *W,
                              const float *bias, float *out, int64_t ldo, int32_t M, void *stream);
/* round 6: a three-layer head Sequential(Linear, LeakyReLU(0.01), Linear, LeakyReLU, Linear) on 256-channel rows in ONE launch (models/ehem.py:113-121:
 * prob_pred_mlp1 256 -> 256 -> 256 -> 255 and pre_attn_mlp 256 -> 256 -> 240 -> 240): out[out_map ? out_map[m] : m][0 .. N) = head(x[in_map ? in_map[m] : m]),
 * rows with out_map[m] < 0 dropped.  x: fp32 [n_src][ldx]; W: scp_swin_post_attn_weight_bytes() bytes with three tiled [256][256] matrices (hi planes at
 * m * 131072 bytes, lo planes at the same offsets in the second half; layers 2, 3: columns in accumulator order; unused rows / columns zero); bias [768];
 * N % 4 == 0, N <= 256, 16-byte aligned output rows.  Every row's result is independent of what else is in the launch. */
SCP_API int scp_mlp3_rows(const float *x, int64_t ldx, int64_t n_src, const int64_t *in_map, const void *W, const float *bias, float *out, int64_t ldo,
                          const int64_t *out_map, int32_t M, int32_t N, void *stream);

/* Keys and values handed from the projection to the window attention as bf16 hi / lo PLANES in the layout of the attention kernel's own
 * LDS tiles (swin_transformer.py:443-501; round 3).  planes: [4][Tp][256] bf16 = K hi, K lo, V^T hi, V^T lo for Tp rows of the packed
 * layout (Tp % 32 == 0; windows of 512 rows):
 *   K   [row][4 heads][64 d], the eight 16-byte chunks of a head's 128 bytes at position chunk ^ (row & 7);
 *   V^T [32-row block][head][32 super-rows of 128 B]: head dim d, 8-key chunk c at super-row d >> 1, slot ((d & 1) * 4 + c) ^ ((d >> 1) & 7),
 *       the block's keys in the order p = 16 c' + 8 h + j  <->  key 16 c' + 4 h + (j & 3) + 8 (j >> 2).
 * The attention kernel copies whole 1 KiB pieces of them into LDS by LDS-DMA: no conversion, no staging registers.
 *   scp_swin_kv_planes              : fp32 k, v [rows][ldkv] -> planes (a plain conversion pass; rows % 32 == 0)
 *   scp_swin_ln_qkv                 : scp_swin_ln_linear for N = 768 (query | key | value; q fp32 [M][ldq]) or N = 512 (key | value, q NULL)
 *                                     writing the key / value heads as planes straight from the accumulators (M % 128 == 0, Tp >= M)
 *   scp_swin_attention_packed_planes: scp_swin_attention_packed(_split) on (q fp32, planes); out fp32 [rows][256] or ohi / olo planes
 * All three give the bits of the fp32 hand-over (scp_swin_ln_linear + scp_swin_attention_packed).  * valid (device fp32 [rows], may be NULL): 1 for real rows, 0 for window padding - a query tile (128 aligned rows) whose first row is
 * padding is skipped and its output rows are not written.
 *
 * The attention OUTPUT travels to scp_swin_post_attn the same way: with ldo (scp_swin_attention_packed_planes) / ldo_in (scp_swin_post_attn)
 * = SCP_LDO_FRAG the o planes are the linear image of the post-attention kernels' B fragments instead of rows:
 *   o   [128-row tile][32 chunks of 8 channels][128 rows][8 bf16] per plane (hi, lo): channel c of row r at element
 *       (((r >> 7) * 32 + (c >> 3)) * 128 + (r & 127)) * 8 + (c & 7); 512 bytes per row as before, whole tiles: ceil(M / 128) * 128 * 256
 *       elements per plane, 16-byte aligned.
 * A lane of the consumer (row = lane & 31, half = lane >> 5) loads the fragment of k-step s - chunk 2 s + half - with one 16-byte load, a
 * wave's load reads 2 x 512 contiguous bytes, and every store of the attention kernel writes whole lines.  Same values as the row-major
 * planes [M][ldo], which stay available (a stride >= 256) for callers that feed other consumers. */
#define SCP_LDO_FRAG 0
SCP_API int scp_swin_kv_planes(const float *k, const float *v, int64_t ldkv, int64_t rows, void *khi, void *klo, void *vthi, void *vtlo, void *stream);
SCP_API int scp_swin_ln_qkv(const float *x, int64_t ldx, const float *valid, const void *Whi, const void *Wlo, const float *bias, const float *wbeta,
                            float eps, float *q, int64_t ldq, void *planes, int64_t Tp, int32_t M, int32_t N, void *stream);
SCP_API int scp_swin_attention_packed_planes(const float *q, const void *khi, const void *klo, const void *vthi, const void *vtlo,
                                             const float *bias_table, const int32_t *wtab, int32_t total_windows, int32_t shift, int32_t ldq,
                                             float *out, void *ohi, void *olo, int64_t ldo, const float *valid, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SCP_H */
