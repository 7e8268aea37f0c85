/* openpifpaf_amd -- C ABI of the MI355X-native CifCaf decode path.
 *
 * This header is the drop-in boundary.  Every entry point replaces one piece
 * of the reference's native decoder interface, the TorchScript registrations
 * in /root/reference/src/openpifpaf/csrc/src/module.cpp:19-118 (cited per
 * function below as "ref: module.cpp:<line>").  Signatures are plain C: raw
 * pointers, sizes and a HIP stream passed as void*.  No torch types.
 *
 * Conventions
 *  - "dev" pointers are HIP device pointers (MI355X HBM); "host" pointers are
 *    ordinary host memory.  All tensors are dense, row-major, float32 unless
 *    stated otherwise, and batched: the leading dimension is the image.
 *  - Field layouts are the reference's CompositeField4 layouts
 *    (ref: network/heads.py:290,360-378):
 *      CIF [B, F, 5, H, W]  comps: 0 unused, 1 conf, 2 x, 3 y, 4 scale
 *      CAF [B, A, 8, H, W]  comps: 0 unused, 1 conf, 2 x1, 3 y1, 4 x2, 5 y2, 6 s1, 7 s2
 *  - Work is enqueued on `stream` and NOT synchronised; results are valid once
 *    the stream reaches that point.  No entry point allocates device memory:
 *    the caller owns the workspace (size from opa_cifcaf_workspace_bytes).
 *  - Return value: OPA_OK or an error code; opa_last_error() gives the text.
 *  - Semantics are those of a FRESH reference decoder instance per image
 *    (CifHr revision 1.0): see DESIGN.md "revision".
 */
#ifndef OPENPIFPAF_AMD_H_
#define OPENPIFPAF_AMD_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OPA_OK 0
#define OPA_ERR_INVALID_ARGUMENT 1   /* bad shape / null pointer / bad handle      */
#define OPA_ERR_HIP 2                /* a HIP runtime call or kernel launch failed  */
#define OPA_ERR_UNSUPPORTED 3        /* option the HIP path does not implement      */
#define OPA_ERR_WORKSPACE 4          /* workspace too small                         */
#define OPA_ERR_NO_DEVICE 5          /* no gfx950 device visible                    */

/* out_count of opa_cifcaf_decode: number of valid rows, plus OPA_COUNT_OVERFLOW when poses were dropped for lack
 * of capacity (max_annotations too small), plus OPA_COUNT_FAILED when the image could not be decoded: the association
 * kernel's watchdog fired (a protocol error, never seen outside the test that provokes it; status word -1), or the image's
 * CIF map reaches more tiles than its pool holds (opa_shape::cifhr_pool_tiles; status word -2: decode again with a
 * larger pool).  The image then has 0 rows and its result must not be used.  Both flags travel with the count, so a
 * caller that reads the counts sees them. */
#define OPA_COUNT_OVERFLOW 0x40000000
#define OPA_COUNT_FAILED 0x20000000
#define OPA_COUNT_ROWS(c) ((c) & 0x0FFFFFFF)

/* The reference's process-global tunables (its C++ static members), one field
 * per STATIC_GETSET line of module.cpp:26-32,76-116 plus the constructor
 * constants of cifcaf.cpp:153 / cifcaf.hpp:103.  Defaults in comments. */
typedef struct opa_params {
    double cif_threshold;            /* CifHr::threshold               0.3     cif_hr.cpp:14        */
    int64_t cifhr_neighbors;         /* CifHr::neighbors               16      cif_hr.cpp:13        */
    double seed_threshold;           /* CifSeeds::threshold            0.2     cif_seeds.cpp:11     */
    double caf_threshold;            /* CafScored::default_score_th    0.3     caf_scored.cpp:11    */
    double cif_floor;                /* CafScored cif_floor            0.1     cifcaf.cpp:153       */
    double keypoint_threshold;       /* CifCaf::keypoint_threshold     0.15    cifcaf.cpp:20        */
    double keypoint_threshold_rel;   /* CifCaf::keypoint_threshold_rel 0.5     cifcaf.cpp:21        */
    double nms_suppression;          /* NMSKeypoints::suppression      1e-5    nms_keypoints.cpp:12 */
    double nms_instance_threshold;   /* NMSKeypoints::instance_threshold 0.15  nms_keypoints.cpp:13 */
    double nms_keypoint_threshold;   /* NMSKeypoints::keypoint_threshold 0.15  nms_keypoints.cpp:14 */
    double force_complete_caf_th;    /* CifCaf::force_complete_caf_th  0.001   cifcaf.cpp:24        */
    double occupancy_reduction;      /* Occupancy(reduction, .)        2.0     cifcaf.hpp:103       */
    double occupancy_min_scale;      /* Occupancy(., min_scale)        4.0     cifcaf.hpp:103       */
    int32_t greedy;                  /* CifCaf::greedy                 0       cifcaf.cpp:19        */
    int32_t reverse_match;           /* CifCaf::reverse_match          1       cifcaf.cpp:22        */
    int32_t force_complete;          /* CifCaf::force_complete         0       cifcaf.cpp:23        */
    int32_t block_joints;            /* CifCaf::block_joints           0       cifcaf.cpp:18 (no-op in the reference) */
    int32_t ablation_cifseeds_nms;        /* CifSeeds::ablation_nms          0  cif_seeds.cpp:13  */
    int32_t ablation_cifseeds_no_rescore; /* CifSeeds::ablation_no_rescore   0  cif_seeds.cpp:14  */
    int32_t ablation_caf_no_rescore;      /* CafScored::ablation_no_rescore  0  caf_scored.cpp:12 */
    int32_t ablation_cifhr_skip;          /* CifHr::ablation_skip            0  cif_hr.cpp:15     */
} opa_params;

/* Shapes of one batched decode call. */
typedef struct opa_shape {
    int32_t batch;            /* B images                                           */
    int32_t n_cif;            /* F = number of CIF fields (= number of keypoints K unless n_keypoints says otherwise) */
    int32_t n_caf;            /* A = number of CAF fields = number of bones         */
    int32_t cif_h, cif_w;     /* CIF field height/width                             */
    int32_t caf_h, caf_w;     /* CAF field height/width                             */
    int32_t cif_stride;       /* pixels per CIF cell (meta.stride)                  */
    int32_t caf_stride;       /* pixels per CAF cell                                */
    int32_t max_annotations;  /* capacity of the per-image annotation output        */
    int32_t n_keypoints;      /* K joints per annotation; 0 = n_cif.  K > n_cif is the reference's tracking
                               * setup (decoder/tracking_pose.py:47-80): joints F..K-1 belong to earlier
                               * frames, have no CIF field -- no seeds, no rescoring, no occupancy, no reverse
                               * match from them (cifcaf.cpp:173,225-229,397; caf_scored.cpp:15-18) -- and are
                               * reached only through initial annotations and bones                    */
    int32_t cifhr_pool_tiles; /* capacity, per image, of the high-resolution CIF map, which the decode keeps as a pool
                               * of 32x64-pixel tiles: only tiles the box of an active CIF cell reaches take a slot
                               * (a 20-person 641-px COCO image: ~450 of its 3927).  0 = automatic: every tile where
                               * the whole map is at most 32 MB per image (nothing can run out), else an eighth of the
                               * map and at least 1024 tiles, plus ONE spill region shared by the batch that holds what
                               * a single image's pool cannot (the rest of a whole map); -1 = every tile (the dense
                               * map's size: can never run out); > 0 = exactly that many, no spill region.  An image
                               * that reaches more tiles than pool + spill region hold is not decoded wrongly: its
                               * count carries OPA_COUNT_FAILED and its status word is -2 (decode it again with -1).  */
} opa_shape;

/* ---- library ------------------------------------------------------------ */
/* The structs above are passed by pointer and have grown over time (opa_shape::cifhr_pool_tiles is the latest field): a
 * caller built against another header would make the library read past its struct.  Check once at start-up that
 * opa_abi_version() == OPA_ABI_VERSION and opa_shape_bytes() == sizeof(opa_shape), opa_params_bytes() == sizeof(opa_params). */
#define OPA_ABI_VERSION 9             /* 9: opa_pre_image, opa_preprocess_u8, opa_preprocess_workspace_bytes */
int opa_abi_version(void);
size_t opa_shape_bytes(void);
size_t opa_params_bytes(void);
size_t opa_debug_bytes(void);
const char* opa_version(void);
const char* opa_last_error(void);            /* thread-local, never NULL            */
int opa_device_count(void);                  /* number of visible gfx950 devices    */

/* ref: module.cpp:19-21  torch.ops.openpifpaf.set_quiet(bool) */
void opa_set_quiet(int quiet);

/* Order of seeds with EQUAL scores (ref: cif_seeds.cpp:94,118: an unstable std::sort, so the reference's order is
 * whatever libstdc++'s introsort leaves -- it decides which of two equally scored seeds is grown first).
 *   1 (default)  libstdc++'s order, reproduced on the device for the images that have such seeds (float32 fields of a
 *                network practically never do; fields rounded to bfloat16 do) -- introsort's partitions and, since round 6,
 *                its heapsort branch (std::__partial_sort for a segment at the depth limit).  The workspace view "seed_ties"
 *                (int32 [B]) says per image: 0 no equal scores, 1 re-ordered (-1: a protocol failure of the pass, never seen:
 *                the image keeps the order below).
 *   0            cell index ascending (field, row, column) -- one launch less.
 *   2            like 1 (rounds 4-5: "with the pass inside the association kernel" -- that is a decoder's own choice now,
 *                opa_cifcaf_set_tie_placement, and the default).
 * Process-global like the reference's statics; the environment variable OPA_SEED_TIES=index / libstdcxx-fused selects 0 / 2
 * when this function was never called (read once, when the library is loaded). */
void opa_set_seed_tie_order(int order);
int opa_get_seed_tie_order(void);

/* The reference keeps its tunables in process-global statics that are set
 * before decoders are built (ref: decoder/factory.py:52-82, decoder/cifcaf.py:175-211).
 * opa_get_params/opa_set_params are that global; every call also accepts an
 * explicit opa_params* (NULL = use the global). */
void opa_default_params(opa_params* out);
void opa_get_params(opa_params* out);
int opa_set_params(const opa_params* in);

/* ---- CifCaf decoder object ---------------------------------------------- */
/* ref: module.cpp:25,34  torch.classes.openpifpaf_decoder.CifCaf(n_keypoints, skeleton)
 * skeleton_host: int64 [n_bones, 2], 0-based joint indices, CAF field order
 * (ref: decoder/cifcaf.py:119-122).  The handle owns a small device copy of
 * the skeleton and its adjacency; it holds no per-call state, so one handle may be used from several streams.  A decode
 * queues all its work on the caller's stream. */
typedef struct opa_cifcaf opa_cifcaf;
int opa_cifcaf_create(opa_cifcaf** out, int32_t n_keypoints,
                      const int64_t* skeleton_host, int32_t n_bones);
void opa_cifcaf_destroy(opa_cifcaf* dec);
/* ref: module.cpp:41-53 (pickle state = (n_keypoints, skeleton)) */
int opa_cifcaf_get_state(const opa_cifcaf* dec, int32_t* n_keypoints,
                         int64_t* skeleton_host /* [n_bones,2] or NULL */, int32_t* n_bones);

/* Where the pass that puts seeds of EQUAL score into the reference's order runs for THIS decoder's decodes (seed tie
 * order 1, see opa_set_seed_tie_order): 1 = inside the association kernel, every image its own ties; 0 = a launch of its own
 * (its time then shows up under its own name); -1 (default) = automatic, which since round 6 means inside the kernel -- measured
 * shorter for one decode at a time as well as for several in flight.  The results are the same bit for bit. */
int opa_cifcaf_set_tie_placement(opa_cifcaf* dec, int32_t inside_association);

/* A/B and test switches of ONE decoder handle (no reference counterpart; the reference's tunables are opa_params).  None of
 * them changes a result: they select between exact variants of the kernels, shorten the watchdog, or switch measurements on.
 * opa_default_debug() = the library's defaults with the environment variables named below applied -- the environment is read
 * ONCE, when the library is loaded, never during a decode (rounds 2-5 looked 20 variables up at every launch, and tests
 * flipped them mid-process next to running decode lanes).  opa_cifcaf_set_debug() copies the struct into the handle; a decode
 * reads only that copy. */
typedef struct opa_debug {
    int32_t stage_worklist;        /* 1: tiles of the CIF map through a work list, seeds from candidate lists (round 6); 0: round 5's
                                    *    per-plane tile kernel and a seed fill that streams the field      OPA_STAGE_WORKLIST      */
    int32_t scored_one_pass;       /* 1: a force-complete decode builds both CAF list sets from ONE read of the field (round 6);
                                    *    0: two passes                                                       OPA_SCORED_ONE_PASS   */
    int32_t assoc_growers;         /* 0 = as many growing waves as fit; n: at most n (other interleavings) OPA_ASSOC_GROWERS      */
    int32_t assoc_bbox;            /* 1: list scans skip chunks whose box misses the window                  OPA_ASSOC_BBOX         */
    int32_t assoc_dedup;           /* 1: later seeds of an occupancy cell already seen are dropped           OPA_ASSOC_DEDUP        */
    int32_t assoc_prededup;        /* 1: ... by the whole workgroup before the coordinator starts            OPA_ASSOC_PREDEDUP     */
    int32_t assoc_predict;         /* 1: joint boxes predicted from single cells of the raw CAF field        OPA_ASSOC_PREDICT      */
    float assoc_predict_min_v;     /* 0.5: seeds below this confidence grow without that walk                OPA_ASSOC_PREDICT_MINV */
    float assoc_predict_th;        /* 0.3: raw CAF confidence a predicted bone needs                         OPA_ASSOC_PREDICT_TH   */
    int32_t assoc_collide;         /* 1: a growth that runs into an earlier candidate's joint box is stopped OPA_ASSOC_COLLIDE      */
    int32_t assoc_collide_shift;   /* 1: ... only near the centre of that box (0: anywhere inside, round 4)  OPA_ASSOC_COLLIDE_SHIFT */
    int32_t assoc_inherit;         /* 1: a candidate inherits the predictions of growths stopped for it      OPA_ASSOC_INHERIT      */
    int32_t assoc_lookahead;       /* 1: large skeletons: the next person's first seed enters the pool early OPA_ASSOC_LOOKAHEAD    */
    int32_t assoc_timing;          /* 0; 1: the coordinator fills its per-phase tick counters                OPA_ASSOC_TIMING       */
    int32_t assoc_persistent;      /* 0 = automatic: in a batch of more images than the chip has compute units the association
                                    *    workgroups take their images from a queue, most seeds first (round 6); 1: always;
                                    *    -1: never (workgroup b = image b)                                   OPA_ASSOC_PERSISTENT   */
    int32_t fc_split;              /* 0 = automatic; n: force-complete workgroups per image                  OPA_FC_SPLIT           */
    int64_t assoc_watchdog_ticks;  /* 1e8 (one second): 10-ns ticks after which a wait inside the association kernel gives up
                                    *    and the image is flagged OPA_COUNT_FAILED                           OPA_ASSOC_WATCHDOG_TICKS */
} opa_debug;
void opa_default_debug(opa_debug* out);
int opa_cifcaf_set_debug(opa_cifcaf* dec, const opa_debug* in);
int opa_cifcaf_get_debug(const opa_cifcaf* dec, opa_debug* out);

/* Bytes of device workspace opa_cifcaf_decode needs for `shape`
 * (0 and an error text if the shape is invalid).
 *
 * The workspace may hold anything when it is first used.  Between calls it carries one piece of
 * state: a 256-byte header plus a bitmap of the 32x64 tiles of the high-resolution map the previous
 * call wrote to, so that tiles no CIF cell touches and that are already zero are not written again
 * (the per-tile form of the reference's lazy clear, cif_hr.cpp:97-121).  The bitmap is trusted only
 * while the header matches the layout of the call.  So: do not write into a workspace between the calls that use
 * it; after lending the memory to anything else, overwrite its first 256 bytes (hipMemset 0) --
 * that alone makes the next call treat every tile as dirty. */
size_t opa_cifcaf_workspace_bytes(const opa_shape* shape);

/* The same for one set of tunables (NULL = the process-global ones): without params->force_complete the second
 * CAF list set, its chunk boxes and counters -- about 30 % of the workspace -- are left out (they sit at the end of
 * the layout; every other offset is unchanged).  opa_cifcaf_decode with force_complete set refuses such a
 * workspace (OPA_ERR_WORKSPACE).  opa_cifcaf_workspace_bytes(shape) is the size that serves every setting. */
size_t opa_cifcaf_workspace_bytes_for(const opa_shape* shape, const opa_params* params);

/* ref: module.cpp:35-36  CifCaf.call / CifCaf.call_with_initial_annotations,
 * i.e. cifcaf.cpp:116-262, batched over B images and reading the field
 * tensors where the network wrote them (device memory; the reference
 * hard-requires CPU tensors, cifcaf.cpp:137-138).
 *
 *  cif_dev  [B,F,5,H,W], caf_dev [B,A,8,H,W]: read by the kernels the call queues on `stream` -- the CAF tensor by the LAST of
 *                   them too (the association kernel reads single cells of it, round 5): both have to stay as they are until
 *                   the work queued by this call has run (the call itself returns at once)
 *  initial_dev      optional [B, n_initial, K, 4] (v,x,y,s) or NULL
 *  initial_ids_dev  optional int64 [B, n_initial] or NULL
 *  out_dev          [B, max_annotations, K, 4] (v,x,y,s)   (ref: cifcaf.cpp:246-258), K = the decoder's n_keypoints
 *  out_ids_dev      int64 [B, max_annotations]             (ref: cifcaf.cpp:259)
 *  out_count_dev    int32 [B]  OPA_COUNT_ROWS(c) = number of valid rows of each image (<= max_annotations, in the
 *                   reference's output order, score descending); rows behind them are not written.  The
 *                   OPA_COUNT_OVERFLOW bit is set when the annotation capacity was too small: the poses the
 *                   seed loop produced after the first max_annotations (in seed order, cifcaf.cpp:206-231) were
 *                   dropped before keypoint NMS, and the workspace's "status" buffer holds how many.
 *                   OPA_COUNT_FAILED: see above (opa_debug::assoc_watchdog_ticks = the watchdog in 10-ns
 *                   ticks, default 1e8 = one second; tests shorten it to provoke the failure).
 */
int opa_cifcaf_decode(const opa_cifcaf* dec, const opa_shape* shape, const opa_params* params,
                      const float* cif_dev, const float* caf_dev,
                      const float* initial_dev, const int64_t* initial_ids_dev, int32_t n_initial,
                      void* workspace_dev, size_t workspace_bytes,
                      float* out_dev, int64_t* out_ids_dev, int32_t* out_count_dev,
                      void* stream);

/* ref: module.cpp:37-39  CifCaf.get_cifhr() -> (Tensor[F,Hhr,Whr], revision).
 * The decode keeps the high-resolution map as a pool of tiles (opa_shape::cifhr_pool_tiles); this call writes the map of
 * image `image` of the LAST opa_cifcaf_decode into that workspace as the dense float32 [n_cif, rows, cols] array the
 * reference returns -- out_dev, device memory of n_cif * rows * cols floats (rows / cols: opa_cifcaf_cifhr_view) --
 * asynchronously on `stream`.  Cell content is the reference buffer's content at revision 1.0: 0.0 = never touched,
 * otherwise 1.0 + accumulated confidence. */
int opa_cifcaf_get_cifhr(const opa_shape* shape, const void* workspace_dev, int32_t image, float* out_dev, void* stream);

/* Geometry of that array: rows = (cif_h - 1) * stride + 1, cols likewise; pitch = cols; revision = 1.0.
 * offset_floats: SIZE_MAX -- the map is NOT a dense array inside the workspace any more (rounds 1-3 returned its offset;
 * a caller that still indexes the workspace with it fails loudly instead of reading tile pools): use opa_cifcaf_get_cifhr. */
int opa_cifcaf_cifhr_view(const opa_shape* shape, size_t* offset_floats,
                          int32_t* rows, int32_t* cols, int32_t* pitch, double* revision);

/* Locates an intermediate buffer of the last opa_cifcaf_decode inside the workspace
 * (debugging / tests; the reference exposes its intermediates through the utility
 * classes of module.cpp:66-117).  what: "tile_bitmaps" (u32 [2][B*F][words]: tiles of the map written by
 * the previous / by this call), "cifhr", "seed_count", "seed_f", "seed_vxys", "seed_cell", "seed_ties",
 * "lists", "list_counts", "lists_fc", "list_counts_fc", "list_bbox" (f32 [B,A,2,C,4], C = min(ceil(caf_h*caf_w/64),
 * 255): xmin, xmax, ymin, ymax of the (x1, y1) columns of the first min(C, 16) chunks of 64 entries of every "lists"
 * list -- the rest of a list's C boxes is not written; an empty chunk: +inf, -inf, +inf, -inf), "list_bbox_fc" (the
 * boxes of ALL C chunks of every "lists_fc" list; written only by a force-complete decode), "occupancy",
 * "annotation_scratch", "status" (int32 [B]: poses dropped for lack of capacity; -1: the kernel's watchdog
 * fired; -2: the image's CIF map did not fit its tile pool), "cifhr_slots" (int32 [B, n_cif, tiles per plane]: slot of a map
 * tile in its image's pool, negative: no cell reaches the tile), "cifhr_overflow" (int32 [B]), "assoc_stats" (int32 [B,24] per image: 0 growths started, 1 poses accepted, 2 growths stopped because
 * their seed died, 3 finished growths dropped for the same reason, 4 growths stopped or given up on a prediction
 * (the seed stays pooled), 5 seeds handed out after having been predicted dead, 6 pool refills, 7 seeds,
 * 8 ticks until the growth phase ended, 9 ticks of the kernel, 10 sum of the growers' busy ticks, 11 list
 * scans, 12 coordinator ticks spent in iterations that only waited for the head's growth, 13 growers,
 * 14 poses stored, 15 coordinator iterations, 16 of them waiting, 17/18/19 ticks in commits / refills / hand-outs,
 * 20 ticks of the refills spent waiting for the growers' occupancy marks, 21 joint boxes published from PREDICTIONS (a growth's walk over
 * single cells of the raw CAF field before its search; round 5) and 22 seeds that entered the pool ahead of the scan (large skeletons' lookahead;
 * round 5) -- in diagnostic builds both also carry scan timing --, 23 seeds
 * dropped as later seeds of an occupancy cell already seen -- by the workgroup's pass over the seed list before the pool sees it
 * (round 5) and, for what that pass admits, at the refills; ticks are 10 ns; the tick
 * counters 12 and 17-20 are filled only with opa_debug::assoc_timing: each costs clock reads in the coordinator's loop), "assoc_trace" (int32 [B,64,4]: for the first
 * 64 accepted poses of an image the tick of the commit, of the hand-out and of the end of the growth, and
 * seed index | grower << 24), "assoc_queue" (int32 [B + 1]: batches of more images than compute units -- the images by seed count,
 * most first, then the queue's head; round 6), "cifhr_work" (int2 [..]: the tile kernel's work list, round 6).
 * The three "*_fc" regions lie at the END of the layout: their offsets are only inside a workspace of
 * opa_cifcaf_workspace_bytes() (or ..._bytes_for() with force_complete set); a workspace sized without the flag
 * ends before them -- do not dereference them there. */
int opa_cifcaf_workspace_view(const opa_shape* shape, const char* what,
                              size_t* offset_bytes, size_t* size_bytes);

/* ---- stage-level entry points (openpifpaf_decoder_utils) ---------------- */
/* ref: module.cpp:75-84  CifHr.reset + CifHr.accumulate (cif_hr.cpp:28-121).
 *  cifhr_dev [B, F, rows, pitch] with rows=(H-1)*stride+1, pitch from opa_cifhr_pitch();
 *  scratch_dev: opa_cifhr_scratch_bytes() bytes. */
int32_t opa_cifhr_pitch(int32_t cif_w, int32_t stride);
size_t opa_cifhr_scratch_bytes(int32_t batch, int32_t n_cif, int32_t cif_h, int32_t cif_w);
int opa_cifhr_accumulate(const float* cif_dev, int32_t batch, int32_t n_cif, int32_t cif_h, int32_t cif_w,
                         int32_t stride, double min_scale, double factor, const opa_params* params,
                         float* cifhr_dev, void* scratch_dev, size_t scratch_bytes, void* stream);

/* ref: module.cpp:86-94  CifSeeds(cifhr, revision).fill(cif, stride) + get()
 * (cif_seeds.cpp:33-66,93-114).  Output sorted by v descending; equal scores in
 * the order the reference's std::sort leaves them in (opa_set_seed_tie_order).
 *  seed_f_dev int32 [B, cap], seed_vxys_dev [B, cap, 4] (v,x,y,s), seed_count_dev int32 [B],
 *  cap = F*H*W;  scratch_dev: opa_cifseeds_scratch_bytes() bytes. */
size_t opa_cifseeds_scratch_bytes(int32_t batch, int32_t n_cif, int32_t cif_h, int32_t cif_w);
int opa_cifseeds_fill(const float* cif_dev, int32_t batch, int32_t n_cif, int32_t cif_h, int32_t cif_w,
                      int32_t stride, const float* cifhr_dev, const opa_params* params,
                      int32_t* seed_f_dev, float* seed_vxys_dev, int32_t* seed_count_dev,
                      void* scratch_dev, size_t scratch_bytes, void* stream);

/* ref: module.cpp:96-102  CifDetSeeds(cifhr, revision).fill(cifdet_field, stride) + get()
 * (cif_seeds.cpp:69-90,117-139).  field_dev [B, F, 6, H, W]; same ordering rule as opa_cifseeds_fill.
 *  seed_f_dev int32 [B, cap], seed_vxywh_dev [B, cap, 5] (v,x,y,w,h), seed_count_dev int32 [B],
 *  cap = F*H*W;  scratch_dev: opa_cifseeds_scratch_bytes() bytes. */
int opa_cifdetseeds_fill(const float* field_dev, int32_t batch, int32_t n_fields, int32_t field_h, int32_t field_w,
                         int32_t stride, const float* cifhr_dev, const opa_params* params,
                         int32_t* seed_f_dev, float* seed_vxywh_dev, int32_t* seed_count_dev,
                         void* scratch_dev, size_t scratch_bytes, void* stream);

/* ref: module.cpp:104-111  CafScored(cifhr, revision, score_th, cif_floor).fill(caf, stride, skeleton) + get()
 * (caf_scored.cpp:29-104).  Lists keep the reference's raster (j,i) order.
 *  skeleton_dev int64 [A,2] 0-based (device);  score_th < 0 -> params->caf_threshold
 *  lists_dev [B, A, 2(dir: 0 forward, 1 backward), 7, cap] planes (c,x1,y1,x2,y2,s1,s2), cap = caf_h*caf_w
 *  counts_dev int32 [B, A, 2] */
int opa_cafscored_fill(const float* caf_dev, int32_t batch, int32_t n_caf, int32_t caf_h, int32_t caf_w,
                       int32_t stride, const float* cifhr_dev, int32_t n_cif, int32_t cif_h, int32_t cif_w,
                       int32_t cif_stride, const int64_t* skeleton_dev, double score_th, double cif_floor,
                       const opa_params* params, float* lists_dev, int32_t* counts_dev, void* stream);

/* ref: module.cpp:55  torch.ops.openpifpaf_decoder.grow_connection_blend(caf[n,7], x, y, s, filter_sigmas, only_max)
 * (cifcaf.cpp:32-113).  rows_dev: device [n,7] row list; out_host[4] = (x, y, s, v).
 * Synchronous (copies the result back). */
int opa_grow_connection_blend(const float* rows_dev, int32_t n, double x, double y, double s,
                              double filter_sigmas, int32_t only_max, double* out_host, void* stream);

/* ---- CifDet decoder -------------------------------------------------------- */
/* ref: module.cpp:57-62  torch.classes.openpifpaf_decoder.CifDet().call(cifdet_field, stride)
 * (cifdet.cpp:24-80, CifDetHr cif_hr.cpp:124-150, CifDetSeeds cif_seeds.cpp:69-90,117-139), batched.
 *  field_dev       [B, F, 6, H, W]  comps: 0 unused, 1 conf, 2 x, 3 y, 4 w, 5 h
 *  categories_dev  int64 [B, max_detections]  (1-based field index, cifdet.cpp:61)
 *  scores_dev      [B, max_detections]
 *  boxes_dev       [B, max_detections, 4]  (x0, y0, x1, y1)
 *  counts_dev      int32 [B]
 * max_detections is the reference's static CifDet::max_detections_before_nms (120, cifdet.cpp:16).
 * These are the reference's PRE-NMS candidates.  The IoU NMS, score filter and box conversion that the reference runs in host
 * Python behind them (decoder/cifdet.py:60-91) are opa_cifdet_nms / opa_cifdet_decode_nms below: one more kernel on the same
 * stream, so that only final detections leave the device. */
typedef struct opa_det_shape {
    int32_t batch, n_fields, field_h, field_w, stride, max_detections;
} opa_det_shape;
size_t opa_cifdet_workspace_bytes(const opa_det_shape* shape);
int opa_cifdet_decode(const opa_det_shape* shape, const opa_params* params, const float* field_dev,
                      void* workspace_dev, size_t workspace_bytes,
                      int64_t* categories_dev, float* scores_dev, float* boxes_dev, int32_t* counts_dev,
                      void* stream);

/* ref: decoder/cifdet.py:16-21,60-91  the class attributes of the reference's Python CifDet and what its __call__ does with
 * them after the native call: torchvision batched_nms (nms when by_category is 0) at iou_threshold, scores of suppressed
 * candidates multiplied by `suppression`, candidates kept where the score exceeds instance_threshold, boxes as (x, y, w, h).
 * Defaults in comments; check opa_det_post_bytes() == sizeof(opa_det_post) once at start-up, like the structs above. */
typedef struct opa_det_post {
    double iou_threshold;       /* CifDet.iou_threshold       0.5   compared in double                      */
    double suppression;         /* CifDet.suppression         0.1   applied as a float32 factor             */
    double instance_threshold;  /* CifDet.instance_threshold  0.15  compared as a float32                   */
    int32_t by_category;        /* CifDet.nms_by_category     1     boxes of different categories never suppress each other */
} opa_det_post;
size_t opa_det_post_bytes(void);
void opa_default_det_post(opa_det_post* out);

/* Candidates per image the NMS kernel takes (its suppression matrix lives in LDS: 128 KB of row masks at 1024). */
#define OPA_CIFDET_NMS_MAX 1024

/* The post-processing alone, from candidate arrays laid out as opa_cifdet_decode writes them (counts_dev int32 [B]: valid
 * candidates per image, clamped to 0 .. max_detections; any score order) to
 *  out_categories_dev int64 [B, max_detections], out_scores_dev [B, max_detections],
 *  out_boxes_dev [B, max_detections, 4] (x, y, w, h), out_counts_dev int32 [B]
 * -- the surviving candidates of each image in CANDIDATE order (not re-sorted: the reference masks), rows behind
 * out_counts_dev[b] are not written.  The outputs may be the input arrays.  Greedy NMS in stable descending-score order; IoU
 * from the float32 corners in double, iou = inter / max(area_a + area_b - inter, 1e-12), suppressed when iou > iou_threshold.
 * Against the host model (the package's decoder.CifDet._post, i.e. torchvision's nms / batched_nms):
 *  - by_category 0: the host evaluates the same formula in FLOAT32, threshold included (0.3 becomes 0.30000001).  The kept
 *    set is the host's wherever no pair's IoU lies within float32 rounding of the formula of the threshold (about 1e-6 * IoU).
 *  - by_category 1: the host adds category * (largest coordinate + 1) to the corners instead of comparing categories; that
 *    differs from the category test here by double rounding (1e-13), and where a corner lies below -1, for which the
 *    host's shifted boxes of neighbouring categories can still overlap.  Here different categories never suppress each other.
 * One kernel on `stream`; no device memory beyond the arguments.  post NULL = the defaults.  Above 64 KB of LDS (max_detections
 * beyond about 600) the first call on a device also raises the kernel's LDS limit (hipFuncSetAttribute): make that first call
 * outside a stream capture; later calls and smaller capacities capture freely.
 * max_detections > OPA_CIFDET_NMS_MAX: OPA_ERR_INVALID_ARGUMENT, nothing is queued. */
int opa_cifdet_nms(const opa_det_post* post, int32_t batch, int32_t max_detections,
                   const int64_t* categories_dev, const float* scores_dev, const float* boxes_dev, const int32_t* counts_dev,
                   int64_t* out_categories_dev, float* out_scores_dev, float* out_boxes_dev, int32_t* out_counts_dev,
                   void* stream);

/* opa_cifdet_decode followed by opa_cifdet_nms on the same stream, in the caller's output arrays: on return of the queued work
 * categories_dev / scores_dev / boxes_dev (x, y, w, h) / counts_dev hold the FINAL detections of every image; rows behind
 * counts_dev[b] hold leftovers of the candidates.  Same workspace as opa_cifdet_decode.
 * shape->max_detections > OPA_CIFDET_NMS_MAX: OPA_ERR_INVALID_ARGUMENT, nothing is queued (decode with opa_cifdet_decode and
 * post-process on the host). */
int opa_cifdet_decode_nms(const opa_det_shape* shape, const opa_params* params, const opa_det_post* post,
                          const float* field_dev, void* workspace_dev, size_t workspace_bytes,
                          int64_t* categories_dev, float* scores_dev, float* boxes_dev, int32_t* counts_dev,
                          void* stream);

/* ---- producer-side helper ------------------------------------------------ */
/* Fused convolution epilogue of the field-producing network (no reference counterpart:
 * the reference runs conv -> batch-norm -> ReLU (-> add -> ReLU) as separate PyTorch ops,
 * network/basenetworks.py).  In place on an NHWC activation viewed as [rows, channels]:
 *     x = act(x + bias[channel] (+ residual))
 * dtype: 0 = float32, 1 = float16, 2 = bfloat16; channels must be a multiple of 16 bytes
 * worth of elements; x/residual 16-B aligned; residual may be NULL; relu 0/1. */
int opa_bias_act(void* x_dev, const void* bias_dev, const void* residual_dev,
                 int64_t rows, int32_t channels, int32_t dtype, int32_t relu, void* stream);

/* 1x1 convolution as an MFMA GEMM with the epilogue fused (bfloat16 in/out, f32 accumulate):
 *     out[M,N] = act(A[M,K] * W[N,K]^T + bias[N] (+ residual[M,N]))
 * A = NHWC activation viewed as [B*H*W, C_in], W = conv weight [C_out, C_in].  K % 64 == 0,
 * N % 64 == 0, all pointers 16-B aligned; residual may be NULL. */
int opa_gemm_bias_act_bf16(const void* a_dev, const void* w_dev, const void* bias_dev, const void* residual_dev,
                           void* out_dev, int64_t m, int32_t n, int32_t k, int32_t relu, void* stream);

/* The same GEMM with a fused PROLOGUE on its A operand: A is the raw output of the preceding (3x3)
 * convolution and  A'[m,k] = relu(A[m,k] + a_bias[k])  -- that convolution's bias + ReLU -- is applied while
 * the tile is staged, so its separate epilogue pass (opa_bias_act) disappears:
 *     out[M,N] = act(relu(A + a_bias) * W^T + bias (+ residual)) */
int opa_gemm_pro_bias_act_bf16(const void* a_dev, const void* a_bias_dev, const void* w_dev, const void* bias_dev,
                               const void* residual_dev, void* out_dev, int64_t m, int32_t n, int32_t k,
                               int32_t relu, void* stream);

/* Both of the above for FLOAT16 operands (dtype code 1: a, a_bias, w, bias, residual and out all float16) on v_mfma_f32_32x32x16_f16:
 * the same kernel (csrc/gemm_epilogue.hip) with the element type as its template parameter, the same contract, checks and messages
 * under these names.  float32 accumulation, one rounding to float16 at the store, round to nearest even: what rounds beyond 65504
 * becomes +-inf, NaN stays NaN (also through the ReLU, a select here), a result below 2^-14 keeps its subnormal bits --
 * tensor.to(torch.float16) bit for bit.  The prologue is relu(a + a_bias) in float32 rounded once to float16: opa_bias_act with dtype 1. */
int opa_gemm_bias_act_f16(const void* a_dev, const void* w_dev, const void* bias_dev, const void* residual_dev,
                          void* out_dev, int64_t m, int32_t n, int32_t k, int32_t relu, void* stream);
int opa_gemm_pro_bias_act_f16(const void* a_dev, const void* a_bias_dev, const void* w_dev, const void* bias_dev,
                              const void* residual_dev, void* out_dev, int64_t m, int32_t n, int32_t k,
                              int32_t relu, void* stream);

/* Both of the above in float32 (v_mfma_f32_32x32x2f32, f32 operands and accumulation): the network at the
 * reference's precision.  a_bias_dev may be NULL (no prologue).  K % 32 == 0, N % 64 == 0, pointers 16-B aligned. */
int opa_gemm_bias_act_f32(const float* a_dev, const float* a_bias_dev, const float* w_dev, const float* bias_dev,
                          const float* residual_dev, float* out_dev, int64_t m, int32_t n, int32_t k,
                          int32_t relu, void* stream);

/* The float32 GEMM above on the bfloat16 MFMA pipe with NOTHING of either operand dropped (csrc/gemm_f32x3.hip): a float32 is
 * exactly the sum of three bfloat16 (its 24-bit significand cut into 8 + 8 + 8 bits), so a * b is the sum of nine bf16 x bf16
 * products, each exact in the float32 accumulator.  w3_dev = the weight split on the host ([3][N][K] bfloat16:
 * openpifpaf_amd.fused.split_weight), the activation is split while its tile is staged.  terms = 9: all nine products (the
 * only rounding left is the accumulation's, as in any float32 GEMM); 6: without the three smallest (< 2^-23 of a product each).
 * float32 in, float32 out; K % 64 == 0, N % 64 == 0, pointers 16-B aligned; a_bias_dev / residual_dev may be NULL. */
int opa_gemm_bias_act_f32x3(const float* a_dev, const float* a_bias_dev, const void* w3_dev, const float* bias_dev,
                            const float* residual_dev, float* out_dev, int64_t m, int32_t n, int32_t k,
                            int32_t relu, int32_t terms, void* stream);

/* Two 1x1 convolutions that are added -- the last convolution of a ResNet block and the block's downsampling convolution
 * (reference network/basenetworks.py:71-150: torchvision's Bottleneck, out = relu(bn3(conv3(h)) + downsample(x))) -- as ONE product
 * of the same kernel:  out[B, ho, wo, N] = act([a1 | a2 at stride] * w3cat^T + bias),  a1 [B*ho*wo, k1] (the block's inner
 * activation), a2 [B, h_in, w_in, k2] channels-last (the block's input; output pixel (y, x) reads input pixel (stride*y,
 * stride*x), ho = (h_in - 1) / stride + 1), w3cat = split_weight of the two weights concatenated along K ([3][N][k1 + k2]),
 * a_bias_dev [k1 + k2] or NULL (relu(. + a_bias) on the operand: zeros behind k1 leave the non-negative a2 as it is).  The
 * identity tensor is neither written nor read back.  k1 % 32 == 0, (k1 + k2) % 64 == 0, k2 % 4 == 0, N % 64 == 0. */
int opa_gemm2_bias_act_f32x3(const float* a1_dev, int32_t k1, const float* a2_dev, int32_t k2, int32_t batch, int32_t h_in,
                             int32_t w_in, int32_t stride, const float* a_bias_dev, const void* w3cat_dev, const float* bias_dev,
                             float* out_dev, int32_t n, int32_t relu, int32_t terms, void* stream);

/* 3x3 convolution, padding 1, ANY stride, of an NHWC float32 activation as an implicit GEMM of the split-operand kernel: the
 * strided convolution at the head of ResNet layers 2-4 (reference network/basenetworks.py:71-150: torch.nn.Conv2d -> MIOpen).
 * Column block t = 3 ky + kx of K = 9 c_in holds the channels of input pixel (stride*y - 1 + ky, stride*x - 1 + kx); pixels in
 * the padding are zeros.  x_dev [B, h_in, w_in, c_in] (< 2 GB), w3_dev = split_weight of the weight as [c_out, (ky, kx, c_in)]
 * ([3][c_out][9 c_in] bfloat16: openpifpaf_amd.fused.split_weight_3x3), out_dev [B, ho, wo, c_out], ho = (h_in - 1) / stride + 1.
 * c_in % 64 == 0, c_out % 64 == 0; terms 6 or 9 as above. */
int opa_conv3x3_f32x3(const float* x_dev, const void* w3_dev, const float* bias_dev, float* out_dev, int32_t batch, int32_t h_in,
                      int32_t w_in, int32_t c_in, int32_t c_out, int32_t stride, int32_t relu, int32_t terms, void* stream);

/* The same convolution with a DILATION d >= 1 and padding d (the same kernel: opa_conv3x3_f32x3 is its d = 1 call, bit for bit) --
 * the 3x3 convolutions of a ResNet's block 5 under --resnet-block5-dilation (reference network/basenetworks.py:121-135).  Column
 * block t = 3 ky + kx of K holds the channels of input pixel (stride*y - d + d*ky, stride*x - d + d*kx); pixels in the padding are
 * zeros (a dilation beyond the image leaves the centre tap alone).  w3_dev as above (split_weight_3x3: the layout does not depend
 * on d); out_dev [B, ho, wo, c_out], ho = (h_in - 1) / stride + 1.  c_in % 64 == 0, c_out % 64 == 0, pointers 16-B aligned,
 * dilation >= 1, stride >= 1, terms 6 or 9, (batch * h_in * w_in + dilation * (w_in + 1)) * c_in * 4 < 2^31; anything else:
 * OPA_ERR_INVALID_ARGUMENT before any launch.  batch, h_in or w_in == 0: OPA_OK, nothing runs. */
int opa_conv3x3_dilated_f32x3(const float* x_dev, const void* w3_dev, const float* bias_dev, float* out_dev, int32_t batch, int32_t h_in,
                              int32_t w_in, int32_t c_in, int32_t c_out, int32_t stride, int32_t dilation, int32_t relu, int32_t terms,
                              void* stream);

/* The input max-pool of a ResNet (reference network/basenetworks.py:85-93: MaxPool2d(3, 2, 1) behind the stem) together with the
 * stem's epilogue, one pass over a channels-last activation (csrc/pool.hip):
 *     out[b, y, x, c] = max over the 3x3 window at (2y - 1, 2x - 1) of act(x[b, iy, ix, c] + bias[c])
 * computed as act(max(x) + bias) -- both steps are non-decreasing, so this equals max_pool2d(relu(x + bias), 3, 2, 1) as numbers
 * (the sign of a zero result may differ; without bias and relu the bits are torch's); float32 arithmetic, one rounding to the storage type.  Pixels in the padding never win (the window always holds its centre); a
 * NaN in the window gives NaN.  x_dev [B, h, w, c], out_dev [B, ho, wo, c], ho = (h - 1) / 2 + 1; bias_dev [c] of the same dtype
 * or NULL; dtype 0 = float32, 2 = bfloat16; relu 0/1.  c % 8 == 0, pointers 16-B aligned, stride == 2 (any other is refused),
 * batch * h * w * c elements < 2 GB (32-bit offsets, one thread per output vector); anything else: OPA_ERR_INVALID_ARGUMENT before
 * any launch.  batch, h or w == 0: OPA_OK, nothing runs. */
int opa_maxpool3x3_bias_act(const void* x_dev, const void* bias_dev, void* out_dev, int32_t dtype, int32_t batch, int32_t h, int32_t w,
                            int32_t c, int32_t stride, int32_t relu, void* stream);

/* The same pass with torch's ceil_mode=True output sizes -- the three max-pools of SqueezeNet (reference
 * network/basenetworks.py:461-487: MaxPool2d(3, 2, padding 1, ceil_mode=True)): ho = ceil((h - 1) / 2) + 1, one less if
 * (ho - 1) * 2 >= h + 1 (never for this kernel size, stride and padding), i.e. the size above for odd h and one more for even h,
 * whose last window holds row h - 1 alone; wo likewise.  Same kernel, same arguments, same checks in the same order. */
int opa_maxpool3x3_ceil_bias_act(const void* x_dev, const void* bias_dev, void* out_dev, int32_t dtype, int32_t batch, int32_t h, int32_t w,
                                 int32_t c, int32_t stride, int32_t relu, void* stream);

/* Both expand convolutions of a SqueezeNet Fire module (reference network/basenetworks.py:461-487: torchvision's Fire) with their
 * biases, ReLUs and the concatenation, one launch (csrc/fire.hip):
 *     out[b, y, x, n]         = relu(bias[n]        + sum_c       h[b, y, x, c]           * W1[n, c])            n < c_e1
 *     out[b, y, x, c_e1 + n]  = relu(bias[c_e1 + n] + sum_ky,kx,c h[b, y+ky-1, x+kx-1, c] * W3[n, c, ky, kx])    n < c_e3
 * (outside the image: 0).  h_dev [batch, h, w, c_squeeze] and out_dev [batch, h, w, c_e1 + c_e3] channels-last float32; w_dev the
 * split weights in the kernel's fragment order, 3 * (c_e1 + 9 * c_e3) * c_squeeze bfloat16 (openpifpaf_amd.fused.fire_weight_of);
 * bias_dev [c_e1 + c_e3] float32.  Split-operand arithmetic as opa_gemm_bias_act_f32x3 (terms 6 or 9).  c_squeeze 16, 32, 48 or
 * 64; c_e1 and c_e3 multiples of 64; pointers 16-B aligned; both tensors smaller than 2 GB (32-bit byte offsets); anything else:
 * OPA_ERR_INVALID_ARGUMENT before any launch.  batch, h or w == 0: OPA_OK, nothing runs.  A NaN or +-Inf at pixel p of h gives NaN
 * in every c_e1 channel at p and in every c_e3 channel at the pixels whose 3x3 window holds p, and changes no other output. */
int opa_fire_expand_f32x3(const float* h_dev, const void* w_dev, const float* bias_dev, float* out_dev, int32_t batch, int32_t h, int32_t w,
                          int32_t c_squeeze, int32_t c_e1, int32_t c_e3, int32_t terms, void* stream);

/* A convolution whose window ROWS are the taps of the same implicit GEMM, on an input that is padded IN MEMORY: the 7x7 stride-2
 * stem of a ResNet (reference network/basenetworks.py:71-150) on a 4-channel, zero-padded copy of the image.  x_dev [B, hp, wp, pix]
 * (pix floats per pixel); output pixel (y, x) reads for tap t the tap_floats contiguous floats that begin at input pixel
 * (stride*y + t, stride*x); w3_dev = split_weight of the weight laid out to match ([3][c_out][ntaps * tap_floats];
 * openpifpaf_amd.fused.stem7x7_bias_act_x3 pads the image by 3 + 4 pixels and the weight to 8 rows x 8 columns x 4 channels);
 * out_dev [B, ho, wo, c_out].  tap_floats % 32 == 0, ntaps * tap_floats % 64 == 0, ntaps <= 32, c_out % 64 == 0, x < 2 GB; the caller
 * guarantees that every tap of every output pixel lies inside x. */
int opa_conv_rows_f32x3(const float* x_dev, const void* w3_dev, const float* bias_dev, float* out_dev, int32_t batch, int32_t hp,
                        int32_t wp, int32_t pix, int32_t ho, int32_t wo, int32_t stride, int32_t ntaps, int32_t tap_floats,
                        int32_t c_out, int32_t relu, int32_t terms, void* stream);

/* The 1x1 convolutions of a ShuffleNetV2K unit (reference network/basenetworks.py:186-242) through the same kernel: ANY even k
 * and n, the operand a channel SLICE of a wider channels-last tensor, the result optionally stored into its shuffled position.
 *     out[m, n] = act(a[m, k; a_pitch floats between rows] * w^T + bias)                                   (partner_dev NULL)
 *     out[m, 2n]: out[., 2c] = partner[., c; partner_pitch floats between rows] (bit for bit), out[., 2c + 1] = act(...)[c]
 * -- the latter is channel_shuffle(cat((partner, y), 1), 2) written as contiguous rows.  w3_dev = split_weight of the weight padded
 * with zeros to [N_pad][K_pad], bias_dev [N_pad] padded alike, N_pad / K_pad = n / k rounded up to multiples of 64
 * (openpifpaf_amd.fused._unit_weight_of).  Columns of a row of A from k on contribute exactly zero whatever the memory holds,
 * and nothing behind column k of the last row is read.  a_dev, partner_dev and the pitches on 8 bytes (even), w3_dev, bias_dev and
 * out_dev on 16; a_pitch >= k (at most 2^21), partner_pitch >= n; m < 2^31; terms 6 or 9 as above.  m == 0: OPA_OK, nothing runs. */
int opa_gemm_unit_bias_act_f32x3(const float* a_dev, int64_t a_pitch, const void* w3_dev, const float* bias_dev,
                                 const float* partner_dev, int64_t partner_pitch, float* out_dev,
                                 int64_t m, int32_t n, int32_t k, int32_t relu, int32_t terms, void* stream);

/* The same with an activation code and optionally a residual -- the 1x1 convolutions of a MobileNetV3 block (reference
 * network/basenetworks.py:432-446): act 0 none, 1 ReLU, 2 hardswish (x * min(max(x + 3, 0), 6) / 6 in float32);
 *     out[m, n] = act(a * w^T + bias + residual[m, n; residual_pitch floats between rows])                 (residual_dev not NULL)
 * the residual read once, on 8 bytes with an even pitch >= n like the partner.  A residual together with a partner is refused
 * (OPA_ERR_INVALID_ARGUMENT, nothing runs).  act 0 / 1 without a residual are opa_gemm_unit_bias_act_f32x3's own kernels. */
int opa_gemm_unit_act_f32x3(const float* a_dev, int64_t a_pitch, const void* w3_dev, const float* bias_dev,
                            const float* partner_dev, int64_t partner_pitch, const float* residual_dev, int64_t residual_pitch,
                            float* out_dev, int64_t m, int32_t n, int32_t k, int32_t act, int32_t terms, void* stream);

/* The same with two more activation codes, each with one parameter -- MobileNetV2's ReLU6 (reference network/basenetworks.py:407-430)
 * and the LeakyReLU of a ShuffleNetV2K unit (network/basenetworks.py:186-268):
 *     act 3 LeakyReLU:    x < 0 ? x * act_param : x                               (act_param: the slope, finite and >= 0)
 *     act 4 clipped ReLU: x < 0 ? 0 : (x > act_param ? act_param : x)             (act_param: the cap, finite and > 0; ReLU6 is 6)
 * both selects in float32 behind the bias, the last operation before the store: NaN stays NaN, and the result is that function of
 * the act 0 result bit for bit.  With a partner the partner's bits pass through as above.  act 0 .. 2 ignore act_param (which must
 * still be finite) and run opa_gemm_unit_act_f32x3's kernels.  A residual together with act 3 or 4 is refused, like everything
 * opa_gemm_unit_act_f32x3 refuses. */
int opa_gemm_unit_actp_f32x3(const float* a_dev, int64_t a_pitch, const void* w3_dev, const float* bias_dev,
                             const float* partner_dev, int64_t partner_pitch, const float* residual_dev, int64_t residual_pitch,
                             float* out_dev, int64_t m, int32_t n, int32_t k, int32_t act, float act_param, int32_t terms, void* stream);

/* The unit mode in bfloat16 (csrc/gemm_unit_bf16.hip): the 1x1 convolutions of a ShuffleNetV2K / ShuffleNetV2 unit, conv5 and the
 * heads of a network cast to bfloat16, one bf16 MFMA per product, float32 accumulation, ONE rounding at the store:
 *     out[m, n]  = bf16_rne(act(sum_k a[m, k] * w[n, k] + bias[n] (+ residual[m, n])))
 *     out[m, 2n]: out[., 2c] = partner[., c] (bits copied), out[., 2c + 1] = the above                      (partner_dev not NULL)
 * a_dev: bf16 [m, k] with a_pitch bf16 ELEMENTS between rows (a channel slice of a wider channels-last tensor); partner_dev /
 * residual_dev: bf16 [m, n] with their pitches, never both.  w_dev: bf16 [N_pad][K_pad], bias_dev: FLOAT32 [N_pad] -- n and k
 * rounded up to multiples of 64, padded with zeros (a bf16 bias upcast, zeros where there is none).  out_dev: dense bf16.
 * Any even n and k; m < 2^31; k <= a_pitch <= 2^21; partner / residual pitch >= n, even.  a_dev, partner_dev and residual_dev on
 * 4 bytes, w_dev, bias_dev and out_dev on 16: the kernel issues no access wider than the launch's pointers and pitches allow.
 * Columns from k on contribute exactly zero whatever the memory behind a row holds, and no byte behind column k of the last row is
 * read.  act and act_param as opa_gemm_unit_actp_f32x3 (0 none, 1 ReLU, 2 hardswish, 3 LeakyReLU(slope), 4 ReLU clipped at the
 * cap), applied in float32 before the rounding; a residual together with a partner, or with act 3 / 4, is refused.
 * m == 0: OPA_OK, nothing runs. */
int opa_gemm_unit_actp_bf16(const void* a_dev, int64_t a_pitch, const void* w_dev, const float* bias_dev,
                            const void* partner_dev, int64_t partner_pitch, const void* residual_dev, int64_t residual_pitch,
                            void* out_dev, int64_t m, int32_t n, int32_t k, int32_t act, float act_param, void* stream);

/* The same for a network cast to FLOAT16: a_dev, w_dev, partner_dev, residual_dev and out_dev float16, bias_dev float32, the same
 * kernel on v_mfma_f32_32x32x16_f16.  Float32 accumulation, bias and activation; ONE round-to-nearest-even conversion at the store:
 * what rounds beyond 65504 is +-inf, NaN stays NaN, subnormal operands and results are kept (tensor.to(torch.float16) bit for bit).
 * The partner's bits pass through untouched.  Arguments, limits, refusals and their order are opa_gemm_unit_actp_bf16's. */
int opa_gemm_unit_actp_f16(const void* a_dev, int64_t a_pitch, const void* w_dev, const float* bias_dev,
                           const void* partner_dev, int64_t partner_pitch, const void* residual_dev, int64_t residual_pitch,
                           void* out_dev, int64_t m, int32_t n, int32_t k, int32_t act, float act_param, void* stream);

/* The 3x3 convolutions of a ResNet cast to bfloat16 (csrc/conv3x3_bf16.hip; reference network/basenetworks.py:71-150 runs them
 * through torch.nn.Conv2d) as an implicit GEMM on the bf16 MFMA, float32 accumulation, ONE rounding at the store:
 *     out[b, oy, ox, co] = bf16_rne(act(sum_{ky,kx,ci} x[b, s*oy - d + d*ky, s*ox - d + d*kx, ci] * w[co][3*ky + kx][ci]
 *                                       + bias[co] (+ residual[b, oy, ox, co])))
 * x_dev: dense channels-last bf16 [batch, h_in, w_in, c_in]; w_dev: bf16 [c_out][9][c_in] (K-major, K = 9 c_in: the convolution's
 * weight permuted to [c_out, ky, kx, c_in]); bias_dev: FLOAT32 [c_out] or NULL (a bf16 folded bias upcast); residual_dev: dense
 * bf16 [batch, ho, wo, c_out] or NULL; out_dev: dense bf16 of that shape, ho = (h_in - 1) / stride + 1 (wo alike).  s = stride 1 or
 * 2; d = dilation = the padding, 1, or 2 or 4 with stride 1; relu 0 / 1 (a select in float32 behind the sums: NaN stays NaN).
 * c_in % 64 == 0, c_out % 64 == 0; x and out each fewer than 2^31 elements; all five pointers 16-B aligned (NULL passes).
 * A tap outside the image is not loaded: the padding contributes exactly zero whatever memory holds, and no address outside x is
 * read.  No workspace, no atomics: equal inputs give equal bits.  batch, h_in or w_in == 0: OPA_OK, nothing runs; everything
 * else outside this contract is OPA_ERR_INVALID_ARGUMENT. */
int opa_conv3x3_act_bf16(const void* x_dev, const void* w_dev, const float* bias_dev, const void* residual_dev, void* out_dev,
                         int32_t batch, int32_t h_in, int32_t w_in, int32_t c_in, int32_t c_out,
                         int32_t stride, int32_t dilation, int32_t relu, void* stream);

/* opa_conv3x3_act_bf16 for a ResNet cast to FLOAT16, on v_mfma_f32_32x32x16_f16: the same kernel with the element type as its template
 * parameter -- x, w, residual and out float16 where the twin has bf16, bias_dev FLOAT32 as there -- and the same contract, checks and
 * messages under this name.  The store is float16's round to nearest even: beyond 65504 +-inf, NaN stays NaN, subnormal results kept. */
int opa_conv3x3_act_f16(const void* x_dev, const void* w_dev, const float* bias_dev, const void* residual_dev, void* out_dev,
                        int32_t batch, int32_t h_in, int32_t w_in, int32_t c_in, int32_t c_out,
                        int32_t stride, int32_t dilation, int32_t relu, void* stream);

/* The GROUPED 3x3 convolution of a ResNeXt cast to bfloat16 (csrc/gconv3x3_bf16.hip; reference network/basenetworks.py:71-150 runs it
 * through torch.nn.Conv2d with groups = 32) as an implicit GEMM per 64-channel chunk on the bf16 MFMA, float32 accumulation, ONE
 * rounding at the store.  As many output as input channels; the group width divides 64, so the 64 output channels of a chunk
 * depend on its 64 input channels alone:
 *     out[b, oy, ox, co] = bf16_rne(act(sum_{ky,kx} sum_{j<64} x[b, s*oy - d + d*ky, s*ox - d + d*kx, 64*(co/64) + j] * w[co][3*ky + kx][j]
 *                                       + bias[co]))
 * x_dev: dense channels-last bf16 [batch, h_in, w_in, channels]; w_dev: bf16 [channels][9][64] (K-major, K = 576): column j of row co
 * holds the weight of input channel 64*(co/64) + j and is ZERO wherever j / group_width != (co % 64) / group_width (the caller packs
 * it so; the kernel multiplies what it is given); bias_dev: FLOAT32 [channels] or NULL (a bf16 folded bias upcast); out_dev: dense
 * bf16 [batch, ho, wo, channels], ho = (h_in - 1) / stride + 1 (wo alike).  s = stride 1 or 2; d = dilation = the padding, 1, or 2
 * or 4 with stride 1; relu 0 / 1 (a select in float32 behind the sums: NaN stays NaN).  channels % 64 == 0; group_width 4, 8, 16, 32
 * or 64 and below channels; x and out each fewer than 2^31 elements; all four pointers 16-B aligned (NULL passes).
 * A tap outside the image is not loaded: the padding contributes exactly zero whatever memory holds, and no address outside x is
 * read.  NON-FINITE VALUES: the off-group weights are zeros that the MFMA does multiply, so a NaN or Inf in an input channel reaches
 * every output channel of the same 32-ALIGNED CHANNEL BLOCK (group_width 4, 8, 16) at the pixels whose window holds it, not only its
 * own group's; with group_width 32 and 64 it reaches only its own group.  No workspace, no atomics: equal inputs give equal bits.
 * The checks in order -- null pointers, alignment, negative sizes, channels, group_width, stride, dilation, x's size, out's size --
 * each with a message of its own; behind them batch, h_in or w_in == 0: OPA_OK, nothing runs; everything else outside this contract
 * is OPA_ERR_INVALID_ARGUMENT. */
int opa_gconv3x3_act_bf16(const void* x_dev, const void* w_dev, const float* bias_dev, void* out_dev,
                          int32_t batch, int32_t h_in, int32_t w_in, int32_t channels, int32_t group_width,
                          int32_t stride, int32_t dilation, int32_t relu, void* stream);

/* opa_gconv3x3_act_bf16 for a ResNeXt cast to FLOAT16, on v_mfma_f32_32x32x16_f16: the same kernel with the element type as its
 * template parameter -- x, w and out float16 where the twin has bf16, bias_dev FLOAT32 as there -- and the same contract (the one on
 * non-finite values included), checks and messages under this name.  The store is float16's round to nearest even: beyond 65504
 * +-inf, NaN stays NaN, subnormal results kept. */
int opa_gconv3x3_act_f16(const void* x_dev, const void* w_dev, const float* bias_dev, void* out_dev,
                         int32_t batch, int32_t h_in, int32_t w_in, int32_t channels, int32_t group_width,
                         int32_t stride, int32_t dilation, int32_t relu, void* stream);

/* The 7x7 RGB stem of a ResNet cast to bfloat16 (csrc/stem7x7_bf16.hip; reference network/basenetworks.py:71-150 runs it through
 * torch.nn.Conv2d) as an implicit GEMM on the bf16 MFMA, float32 accumulation, ONE rounding at the store:
 *     out[b, oy, ox, co] = bf16_rne(act(sum_{ky,kx,ci} x[b, ci, s*oy - 3 + ky, s*ox - 3 + kx] * w[co][ky * 24 + kx * 3 + ci] + bias[co]))
 * x_dev: bf16 [batch, 3, h, w] read WHERE IT LIES: element (b, ci, y, x) at b * x_batch_stride + ci * x_channel_stride +
 * y * x_row_stride + x * x_pixel_stride ELEMENTS from x_dev (NCHW, channels-last, a cropped view: any four positive strides; no copy
 * is made); w_dev: bf16 [c_out][192], K-major, k = ky * 24 + kx * 3 + ci for ky, kx = 0 .. 6 and ci = 0 .. 2, ZEROS in the 45 other
 * columns; bias_dev: FLOAT32 [c_out] or NULL (a bf16 folded bias upcast); out_dev: dense channels-last bf16 [batch, ho, wo, c_out],
 * ho = (h - 1) / stride + 1 (wo alike).  s = stride 1 or 2, padding 3; relu 0 / 1 (a select in float32 behind the sums: NaN stays NaN).
 * c_out % 64 == 0; x fewer than 2^31 elements from the first to the last addressed, out fewer than 2^31 elements; x_dev 2-B, w_dev,
 * bias_dev and out_dev 16-B aligned (NULL passes).  A tap outside the image is not loaded: the padding contributes exactly zero
 * whatever memory holds, an Inf or NaN pixel reaches exactly the windows that hold it, and no address outside x is read.  No
 * workspace, no atomics: equal inputs give equal bits.  The checks in order -- null pointers, alignment, negative sizes, c_out, stride,
 * x's strides, x's extent, out's size -- each with a message of its own; behind them batch, h or w == 0: OPA_OK, nothing runs;
 * everything else outside this contract is OPA_ERR_INVALID_ARGUMENT. */
int opa_stem7x7_act_bf16(const void* x_dev, int64_t x_batch_stride, int64_t x_channel_stride, int64_t x_row_stride,
                         int64_t x_pixel_stride, const void* w_dev, const float* bias_dev, void* out_dev,
                         int32_t batch, int32_t h, int32_t w, int32_t c_out, int32_t stride, int32_t relu, void* stream);

/* opa_stem7x7_act_bf16 for a ResNet cast to FLOAT16, on v_mfma_f32_32x32x16_f16: the same kernel with the element type as its template
 * parameter -- x, w and out float16 where the twin has bf16, bias_dev FLOAT32 as there -- and the same contract, checks and messages
 * under this name.  The store is float16's round to nearest even: beyond 65504 +-inf, NaN stays NaN, subnormal results kept. */
int opa_stem7x7_act_f16(const void* x_dev, int64_t x_batch_stride, int64_t x_channel_stride, int64_t x_row_stride,
                        int64_t x_pixel_stride, const void* w_dev, const float* bias_dev, void* out_dev,
                        int32_t batch, int32_t h, int32_t w, int32_t c_out, int32_t stride, int32_t relu, void* stream);

/* The tail of the first block of a stage of a ResNet cast to bfloat16 (csrc/gemm2_bf16.hip; reference network/basenetworks.py:71-150
 * runs both convolutions through torch.nn.Conv2d): the block's last 1x1 convolution and its downsampling 1x1 convolution as ONE
 * product on the bf16 MFMA, float32 accumulation, ONE rounding at the store -- the identity tensor is never written:
 *     out[b, oy, ox, :] = bf16_rne(act([a1[m, 0:k1] | a2[b, s*oy, s*ox, 0:k2]] * wcat[n, 0:k1+k2]^T + bias[n])),  m = (b*ho + oy)*wo + ox
 * a1_dev: dense bf16 [batch * ho * wo, k1] (the block's inner activation), NULL exactly when k1 == 0 (the strided 1x1 convolution
 * alone); a2_dev: dense channels-last bf16 [batch, h_in, w_in, k2] (the block's input), read at stride s; ho = (h_in - 1) / stride + 1
 * (wo alike); a_bias_dev: bf16 [k1] or NULL -- with it a1 is the RAW output of the preceding convolution and
 * bf16_rne(max(a1[m, k] + a_bias[k], 0)) in float32 is what is multiplied (opa_gemm_pro_bias_act_bf16's arithmetic; a2 is taken as
 * it is), it needs k1 > 0; wcat_dev: bf16 [n][k1 + k2], K-major (both weights side by side); bias_dev: FLOAT32 [n] or NULL (a bf16
 * folded bias upcast); out_dev: dense bf16 [batch, ho, wo, n].  s = stride 1 or 2; relu 0 / 1 (a select in float32 behind the sums:
 * NaN stays NaN).  k1 % 64 == 0, k2 % 64 == 0 and k2 > 0, n % 64 == 0; a2, a1 and out each fewer than 2^31 elements; all six pointers
 * 16-B aligned (NULL passes).  A row of the tile behind the last output pixel is not loaded, and no address outside a1 or a2 is
 * read.  No workspace, no atomics: equal inputs give equal bits.  The checks in order -- null pointers, alignment, negative sizes,
 * k1, k2, n, stride, the three sizes -- each with a message of its own; behind them batch, h_in or w_in == 0: OPA_OK, nothing runs;
 * everything else outside this contract is OPA_ERR_INVALID_ARGUMENT. */
int opa_gemm2_bias_act_bf16(const void* a1_dev, int32_t k1, const void* a2_dev, int32_t k2, int32_t batch, int32_t h_in, int32_t w_in,
                            int32_t stride, const void* a_bias_dev, const void* wcat_dev, const float* bias_dev, void* out_dev,
                            int32_t n, int32_t relu, void* stream);

/* opa_gemm2_bias_act_bf16 for a ResNet cast to FLOAT16, on v_mfma_f32_32x32x16_f16: the same kernel with the element type as its
 * template parameter -- a1, a2, a_bias, wcat and out float16 where the twin has bf16, bias_dev FLOAT32 as there -- and the same
 * contract, checks and messages under this name.  With a_bias_dev, f16_rne(max(a1[m, k] + a_bias[k], 0)) in float32 is what is
 * multiplied (opa_gemm_pro_bias_act_f16's arithmetic).  The store is float16's round to nearest even: beyond 65504 +-inf, NaN stays
 * NaN, subnormal results kept. */
int opa_gemm2_bias_act_f16(const void* a1_dev, int32_t k1, const void* a2_dev, int32_t k2, int32_t batch, int32_t h_in, int32_t w_in,
                           int32_t stride, const void* a_bias_dev, const void* wcat_dev, const float* bias_dev, void* out_dev,
                           int32_t n, int32_t relu, void* stream);

/* 3x3 convolution, stride 1, padding 1, of an NHWC float32 activation as Winograd F(2x2, 3x3) in ONE kernel (input
 * transform -> sixteen float32 MFMA GEMMs -> output transform; csrc/winograd.hip): the bottleneck convolutions of the
 * ResNet trunk (reference network/basenetworks.py:71-150 runs them through torch.nn.Conv2d), 2.25x fewer multiplications
 * than the direct form, float32 arithmetic throughout.
 *  x_dev [B, h, w, c_in], u_dev = the filter transformed and laid out by openpifpaf_amd.winograd.transform_filter for
 *  `variant` (0, 2 and 3: 64 output channels per workgroup, c_in % 16 == 0, c_out % 64 == 0 -- 2 runs eight waves in two
 *  shifts on the same operand (the default of the Python side), 3 the same as persistent workgroups; 1: 32 channels, c_in % 8 == 0, c_out % 32 == 0), out_dev [B, h, w, c_out]; bias_dev [c_out] or NULL; relu 0/1; order 0 = workgroups of one tile block
 *  on one XCD, 1 = workgroups of one channel block on one XCD.  B*h*w*c_in < 2^30; pointers 16-B aligned; any other variant
 *  is refused. */
int opa_conv3x3_winograd_f32(const float* x_dev, const float* u_dev, const float* bias_dev, float* out_dev, int32_t batch,
                             int32_t h, int32_t w, int32_t c_in, int32_t c_out, int32_t relu, int32_t variant,
                             int32_t order, void* stream);

/* The same convolution on the bf16 MFMA pipe with exactly split operands (variant 4 of csrc/winograd.hip): every float32
 * operand is the sum of three bf16 pieces, the six leading piece products are formed (the three left out are below 2^-23 of
 * a product each), accumulation in float32.  u3_dev = the three bf16 planes of the transformed filter laid out by
 * openpifpaf_amd.winograd.split_filter ([c_out / 64][c_in / 16][16][2][3][64][8] bf16).  variant must be 4; c_in % 16 == 0,
 * c_out % 64 == 0, B*h*w*c_in < 2^30; the rest as opa_conv3x3_winograd_f32. */
int opa_conv3x3_winograd_f32x3(const float* x_dev, const void* u3_dev, const float* bias_dev, float* out_dev, int32_t batch,
                               int32_t h, int32_t w, int32_t c_in, int32_t c_out, int32_t relu, int32_t variant,
                               int32_t order, void* stream);

/* Depthwise k x k convolution (k = 3 or 5, stride 1 or 2, padding k/2) of a channels-last activation, with the
 * folded batch-norm bias and optionally ReLU fused (the ShuffleNetV2K unit of the reference,
 * network/basenetworks.py:186-268; MIOpen runs it as a grouped MFMA convolution, ~100x slower).
 *  x_dev [B, h, w, *] with x_pixel_stride elements between pixels (a channel slice of a wider tensor is fine),
 *  w_dev [k*k, channels] (tap-major), bias_dev [channels] or NULL, out_dev [B, ho, wo, *] with out_pixel_stride;
 *  dtype 0 = float32, 2 = bfloat16 (float32 accumulation).  batch * ho must not exceed 65535 (OPA_ERR_INVALID_ARGUMENT). */
int opa_dwconv_bias_act(const void* x_dev, int64_t x_pixel_stride, const void* w_dev, const void* bias_dev,
                        void* out_dev, int64_t out_pixel_stride, int32_t batch, int32_t h, int32_t w,
                        int32_t channels, int32_t k, int32_t stride, int32_t dtype, int32_t relu, void* stream);

/* The same stencil with an activation code: act 0 none, 1 ReLU (both opa_dwconv_bias_act's own kernels, bit for bit),
 * 2 hardswish in float32 (the depthwise convolution of a MobileNetV3 block); any other code is refused. */
int opa_dwconv_act(const void* x_dev, int64_t x_pixel_stride, const void* w_dev, const void* bias_dev,
                   void* out_dev, int64_t out_pixel_stride, int32_t batch, int32_t h, int32_t w,
                   int32_t channels, int32_t k, int32_t stride, int32_t dtype, int32_t act, void* stream);

/* The same stencil with a 7 x 7 window and a dilation (the ShuffleNetV2K options of the reference, network/basenetworks.py:245-400:
 * --shufflenetv2k-kernel, --shufflenetv2k-stage4-dilation): tap (ky, kx) of output (y, x) reads input
 * (y * stride - p + ky * dilation, x * stride - p + kx * dilation), p = (k / 2) * dilation, zeros outside; w_dev [k*k, channels].
 * k 3, 5 or 7; stride 1 or 2; dilation 1, 2 or 4, stride 1 where it is above 1; dtype and act as opa_dwconv_act, whose results it
 * gives bit for bit where both accept the call.  Everything else is refused like there, and nothing is launched. */
int opa_dwconv_dilated_act(const void* x_dev, int64_t x_pixel_stride, const void* w_dev, const void* bias_dev,
                           void* out_dev, int64_t out_pixel_stride, int32_t batch, int32_t h, int32_t w,
                           int32_t channels, int32_t k, int32_t stride, int32_t dilation, int32_t dtype, int32_t act, void* stream);

/* The same stencil with one more activation code -- the depthwise convolutions of a MobileNetV2 block (reference
 * network/basenetworks.py:407-430): act 4, the ReLU clipped at act_param (x < 0 ? 0 : (x > act_param ? act_param : x) in float32,
 * in bfloat16 before the rounding; act_param finite and > 0, ReLU6 is 6).  act 0 .. 2 ignore act_param (which must still be finite)
 * and give opa_dwconv_dilated_act's results bit for bit; act 3 and everything opa_dwconv_dilated_act refuses are refused. */
int opa_dwconv_actp(const void* x_dev, int64_t x_pixel_stride, const void* w_dev, const void* bias_dev,
                    void* out_dev, int64_t out_pixel_stride, int32_t batch, int32_t h, int32_t w,
                    int32_t channels, int32_t k, int32_t stride, int32_t dilation, int32_t dtype, int32_t act, float act_param, void* stream);

/* opa_dwconv_actp for FLOAT16 tensors (x, w, bias and out float16; the depthwise convolutions of a ShuffleNetV2K cast with .half()):
 * the same stencil, float32 accumulation (float64 products for act 2), one round-to-nearest-even conversion at the store -- beyond
 * 65504 +-inf, NaN stays NaN, subnormal results kept.  No dtype argument: the four entry points above keep refusing dtype 1.
 * Every window, stride, dilation and code opa_dwconv_actp accepts is accepted; the checks, their order and their words are its own. */
int opa_dwconv_actp_f16(const void* x_dev, int64_t x_pixel_stride, const void* w_dev, const void* bias_dev,
                        void* out_dev, int64_t out_pixel_stride, int32_t batch, int32_t h, int32_t w,
                        int32_t channels, int32_t k, int32_t stride, int32_t dilation, int32_t act, float act_param, void* stream);

/* The RGB stem of the non-ResNet backbones (reference network/basenetworks.py: ShuffleNetV2K, ShuffleNetV2, MobileNetV2 / V3,
 * SqueezeNet): a direct 3x3 convolution from 3 input channels, padding 1, dilation 1, stride 1 or 2, float32, with the folded bias
 * and the activation applied before the single store (csrc/stem.hip):
 *     out[b, oy, ox, co] = act(sum_t x[b, ci, oy*s - 1 + ky, ox*s - 1 + kx] * w[t][co] + bias[co]),   t = (ky*3 + kx)*3 + ci
 *  x_dev   [batch, 3, h, w] given by four element strides (batch, channel, row, pixel), all positive: NCHW-contiguous,
 *          channels-last (3 floats per pixel) or a cropped view of either; on a 4-byte boundary; read only, never copied;
 *  w_dev   [27][channels_out] tap-major: row t = (ky*3 + kx)*3 + ci holds weight[co][ci][ky][kx] of the [channels_out, 3, 3, 3]
 *          weight (openpifpaf_amd.fused.stem_weight_of);  bias_dev [channels_out] or NULL;  both and out_dev on 16 bytes;
 *  out_dev dense channels-last [batch, ho, wo, channels_out], ho = (h - 1) / stride + 1 (likewise wo).
 * channels_out 16, 24, 32, 42 or 64 (the stems the networks have).  act 0 none, 1 ReLU (x < 0 ? 0 : x), 2 hardswish, 3 LeakyReLU
 * with the slope act_param (>= 0), 4 ReLU clipped at act_param (> 0; ReLU6 is 6); act_param finite whatever the code; a NaN stays
 * a NaN under every code.  A padded tap contributes nothing: an Inf or NaN in x reaches the windows that hold it and no other.
 * Each output is one chain of 27 float64 fma in the order of t, then + bias in float64, one rounding to float32, then act in
 * float32, whatever the sizes: equal inputs give equal bits, and the sum is as good as correctly rounded.
 * x must span fewer than 2^31 elements (first to last addressed) and out hold fewer than 2^31; batch <= 65535 (grid.y).  Anything
 * else: OPA_ERR_INVALID_ARGUMENT before any launch.  batch == 0: OPA_OK, nothing runs. */
int opa_stem3x3_actp(const float* x_dev, int64_t x_batch_stride, int64_t x_channel_stride, int64_t x_row_stride,
                     int64_t x_pixel_stride, const float* w_dev, const float* bias_dev, float* out_dev,
                     int32_t batch, int32_t h, int32_t w, int32_t channels_out, int32_t stride,
                     int32_t act, float act_param, void* stream);

/* Grouped 3x3 convolution, padding 1, dilation 1, stride 1 or 2, as many output as input channels, float32, channels innermost,
 * with the folded batch-norm bias and optionally ReLU (fmaxf) applied before the single store: the middle convolution of a
 * ResNeXt bottleneck (reference network/basenetworks.py:71-150 with torchvision's grouped Bottleneck).
 *     out[b, y, x, co] = act(bias[co] + sum_{t, ci} x[b, y*s - 1 + ky, x*s - 1 + kx, (co / cg) * cg + ci] * wt[t][ci][co])
 *  x_dev [B, h, w, *] with x_pixel_stride floats between pixels (a channel slice of a wider tensor is fine),
 *  wt_dev [9][group_width][channels]: wt[ky*3 + kx][ci][co] = weight[co][ci][ky][kx] of the [channels, group_width, 3, 3] weight,
 *  bias_dev [channels] or NULL, out_dev [B, ho, wo, *] with out_pixel_stride, ho = (h - 1) / stride + 1 (likewise wo).
 * group_width 4, 8, 16, 32 or 64; channels a multiple of it; pixel strides multiples of 4 and >= channels; every pointer on 16
 * bytes; batch <= 65535 (grid.y) and tiles * ceil(channels / 64) of one image < 2^31 (grid.x); offsets are 64-bit, so the
 * tensors may hold 2^31 elements or more.  Anything else: OPA_ERR_INVALID_ARGUMENT before any launch.  batch, h or w == 0:
 * OPA_OK, nothing runs.  The order of every addition depends on group_width alone (no atomics): equal inputs give equal bits. */
int opa_gconv3x3_bias_act_f32(const float* x_dev, int64_t x_pixel_stride, const float* wt_dev, const float* bias_dev,
                              float* out_dev, int64_t out_pixel_stride, int32_t batch, int32_t h, int32_t w, int32_t channels,
                              int32_t group_width, int32_t stride, int32_t relu, void* stream);

/* torch.cat((a, b), 1) followed by channel_shuffle(groups = 2) of the same unit, in one pass over channels-last rows:
 * out[r, 2i] = a[r, i], out[r, 2i+1] = b[r, i]; a / b with their own pixel strides, out dense [rows, 2*half]. */
int opa_channel_interleave(const void* a_dev, int64_t a_pixel_stride, const void* b_dev, int64_t b_pixel_stride,
                           void* out_dev, int64_t rows, int32_t half, int32_t dtype, void* stream);

/* Squeeze-and-excitation of a MobileNetV3 block (torchvision's SqueezeExcitation, which the reference's backbone contains):
 *     x[b, p, c] *= hardsigmoid(w2 . relu(w1 . mean_p x[b, p, .] + b1) + b2)[c]
 * on a channels-last float32 activation x_dev [batch, pixels, *] with x_pixel_stride floats between pixels, in three calls:
 *  opa_se_pool   sums every OPA_SE_POOL_PIXELS pixels of an image into one partial sum per channel (float64, workspace_dev
 *                [batch][ceil(pixels / OPA_SE_POOL_PIXELS)][channels], opa_se_workspace_bytes bytes);
 *  opa_se_gate   adds the partial sums, divides by `pixels`, rounds the mean to float32 and computes gate_dev [batch, channels]
 *                from w1_dev [squeeze, channels], b1_dev [squeeze], w2_dev [channels, squeeze], b2_dev [channels] (float32);
 *                mean_dev [batch, channels] receives the mean as well, or is NULL;
 *  opa_se_scale  multiplies x by the gate in place.
 * The order of every addition depends on the shape alone (no atomics): equal inputs give equal bits.  channels % 4 == 0,
 * x_pixel_stride % 4 == 0 and >= channels, x_dev / workspace_dev / gate_dev on 16 bytes; batch <= 65535,
 * pixels <= 65535 * OPA_SE_POOL_PIXELS, channels <= 8192, squeeze <= 4096. */
#define OPA_SE_POOL_PIXELS 512
size_t opa_se_workspace_bytes(int32_t batch, int64_t pixels, int32_t channels);
int opa_se_pool(const float* x_dev, int64_t x_pixel_stride, int32_t batch, int64_t pixels, int32_t channels,
                void* workspace_dev, size_t workspace_bytes, void* stream);
int opa_se_gate(const void* workspace_dev, size_t workspace_bytes, int32_t batch, int64_t pixels, int32_t channels, int32_t squeeze,
                const float* w1_dev, const float* b1_dev, const float* w2_dev, const float* b2_dev, float* gate_dev, float* mean_dev,
                void* stream);
int opa_se_scale(float* x_dev, int64_t x_pixel_stride, int32_t batch, int64_t pixels, int32_t channels, const float* gate_dev,
                 void* stream);

/* Group norm and the activation behind it, for a ShuffleNetV2K built with --shufflenetv2k-group-norm (reference
 * network/basenetworks.py:376-400: torch.nn.GroupNorm in place of every BatchNorm2d; csrc/groupnorm.hip):
 *     out[b, p, c] = act((x[b, p, c] - mean[b, g]) * rstd[b, g] * gamma[c] + beta[c]),   g = c / (channels / groups),
 * mean and the biased variance over the (channels / groups) x pixels elements of group g of image b, rstd = 1 / sqrt(var + eps).
 *  x_dev    float32 channels-innermost [batch, pixels, *] with x_pixel_stride floats between pixels (a channel slice of a wider
 *           tensor is fine), on an 8-byte boundary;  out_dev likewise with out_pixel_stride.  out_dev == x_dev with equal strides
 *           works in place; any other overlap of the two is undefined (out_dev == x_dev with unequal strides is refused);
 *  gamma_dev, beta_dev  [channels] float32, or NULL (each on its own): 1 and 0;
 *  workspace_dev  opa_groupnorm_workspace_bytes(batch, pixels, channels) bytes on a 16-byte boundary: the partial moments
 *           [batch][ceil(pixels / OPA_GN_CHUNK_PIXELS)][channels] (sum, sum of squares) in float64, then (a, s) [batch][channels].
 * Three launches on the stream: the moments of every chunk of OPA_GN_CHUNK_PIXELS pixels per channel in float64; per (image,
 * group) the chunks added in their order, then the group's channels in their order, mean = sum / n, var = max(sumsq / n - mean^2, 0),
 * rstd = 1 / sqrt(var + (double)eps) in float64 and, rounded to float32 once each, a = gamma * rstd and s = beta - mean * a;
 * out = act(fmaf(x, a, s)) in float32.  The order of every addition depends on the shape alone (no atomics): equal inputs give
 * equal bits.  act and act_param as opa_stem3x3_actp.
 * The checks, in this order, each with its own message: x_dev / out_dev NULL; alignment (x_dev / out_dev 8, gamma_dev / beta_dev 4,
 * workspace_dev 16 bytes); batch < 0 or pixels, channels, groups <= 0; channels % groups; an odd channels / groups; pixel strides odd
 * or below channels; eps not finite or negative; act outside 0 .. 4; act_param not finite, negative with act 3, not positive with
 * act 4; out_dev == x_dev with unequal strides -- then batch == 0: OPA_OK, nothing runs -- then batch > 65535; pixels > 65535 *
 * OPA_GN_CHUNK_PIXELS; channels / groups > 2048; pixels * channels / 2 >= 2^31; workspace_dev NULL, workspace_bytes too small (both
 * OPA_ERR_WORKSPACE; every other refusal is OPA_ERR_INVALID_ARGUMENT).  Nothing is launched by a refused call.
 * opa_groupnorm_workspace_bytes is 0 for a non-positive argument. */
#define OPA_GN_CHUNK_PIXELS 512
size_t opa_groupnorm_workspace_bytes(int32_t batch, int64_t pixels, int32_t channels);
int opa_groupnorm_actp(const float* x_dev, int64_t x_pixel_stride, const float* gamma_dev, const float* beta_dev, float* out_dev,
                       int64_t out_pixel_stride, int32_t batch, int64_t pixels, int32_t channels, int32_t groups, float eps,
                       int32_t act, float act_param, void* workspace_dev, size_t workspace_bytes, void* stream);

/* The head of the field-producing network after its 1x1 convolution, in one pass (ref: network/heads.py:330-378
 * CompositeField4.forward): PixelShuffle(upsample) -> crop -> [B, n_fields, n_components, H, W] float32 -> sigmoid on
 * the n_confidences components after component 0, cell-index offsets on the vector components whose bit is set in
 * vector_offset_mask (x index on the first, y index on the second of each pair), softplus on the n_scales
 * components behind them.
 *  conv_dev  the convolution's output, channels-last [B, hc, wc, n_fields*n_components*upsample^2],
 *            dtype 0 = float32, 1 = float16, 2 = bfloat16
 *  out_dev   float32 [B, n_fields, n_components, H, W], H = hc*upsample - (upsample-1) (likewise W); upsample 1 or 2 */
int opa_head_epilogue(const void* conv_dev, int32_t dtype, int32_t batch, int32_t hc, int32_t wc,
                      int32_t n_fields, int32_t n_components, int32_t upsample, int32_t n_confidences,
                      int32_t n_vectors, uint32_t vector_offset_mask, int32_t n_scales, float* out_dev, void* stream);

/* A head of a network cast to bfloat16 in ONE kernel (csrc/head16.hip; reference network/heads.py:330-378 runs torch.nn.Conv2d,
 * PixelShuffle, a crop and three in-place passes): its 1x1 convolution on the bf16 MFMA, float32 accumulation, and opa_head_epilogue's
 * arithmetic on the float32 sums -- nothing 16-bit is written, the convolution's output is never rounded:
 *     out[b, f, c, y*us + dy, x*us + dx] = field_c(x[m, 0:k] * w[n, 0:k]^T + bias[n]),   m = (b*hc + y)*wc + x, n = (f*C + c)*us^2 + dy*us + dx
 * us = upsample 1 or 2, C = n_components, field_c as opa_head_epilogue defines it (one device function for both), positions of the last
 * us - 1 rows and columns cropped: H = hc*us - (us-1), W likewise.
 *  x_dev     the trunk's output, dense channels-last bf16 [batch, hc, wc, k], k % 64 == 0, read where it lies
 *  w_dev     bf16 [Np][k], K-major, Np = N = n_fields*n_components*us^2 rounded UP to a multiple of 64: rows 0 .. N-1 the convolution's
 *            weight, the rows from N on ZEROS (they are multiplied; their columns are never stored)
 *  bias_dev  FLOAT32 [Np] (a bf16 bias upcast; what stands behind N is read and not used)
 *  out_dev   float32 [batch, n_fields, n_components, H, W], every element written exactly once
 * n_components == 1 + n_confidences + 2*n_vectors + n_scales.  x (batch*hc*wc*k) and out fewer than 2^31 elements each (32-bit element
 * offsets into both; the weight's rows are addressed in 64 bits), N at most 2^31 - 64; x_dev and w_dev 16-B, bias_dev and out_dev 4-B
 * aligned.  A row of the tile behind the last pixel is not loaded, and no address outside x is read.  Plain stores, no workspace, no
 * atomics: equal inputs give equal bits.  The checks in order -- null pointers (all four), alignment, batch < 0, non-positive hc, wc, k,
 * n_fields or n_components, k % 64, upsample, the component counts (none negative), x's size, N, out's size -- each with a message of its
 * own; behind them batch == 0: OPA_OK, nothing runs; everything else outside this contract is OPA_ERR_INVALID_ARGUMENT.  Nothing is
 * launched by a refused call. */
int opa_head_conv_fields_bf16(const void* x_dev, const void* w_dev, const float* bias_dev, float* out_dev,
                              int32_t batch, int32_t hc, int32_t wc, int32_t k,
                              int32_t n_fields, int32_t n_components, int32_t upsample, int32_t n_confidences,
                              int32_t n_vectors, uint32_t vector_offset_mask, int32_t n_scales, void* stream);

/* opa_head_conv_fields_bf16 for a network cast to FLOAT16, on v_mfma_f32_32x32x16_f16: the same kernel with the element type as its
 * template parameter -- x and w float16 where the twin has bf16, bias_dev and out_dev FLOAT32 as there -- and the same contract, checks
 * and messages under this name. */
int opa_head_conv_fields_f16(const void* x_dev, const void* w_dev, const float* bias_dev, float* out_dev,
                             int32_t batch, int32_t hc, int32_t wc, int32_t k,
                             int32_t n_fields, int32_t n_components, int32_t upsample, int32_t n_confidences,
                             int32_t n_vectors, uint32_t vector_offset_mask, int32_t n_scales, void* stream);

/* ---- image preprocessing ------------------------------------------------ */
/* The evaluation pipeline in front of the network (ref: transforms/scale.py:42-63,150-174 RescaleAbsolute,
 * transforms/pad.py:15-112 CenterPad / CenterPadTight, transforms/__init__.py:26-33 ToTensor + Normalize) for a whole batch of
 * packed uint8 RGB frames of any sizes, in at most two kernel launches: a horizontal resampling pass into a uint8
 * intermediate (only for images whose width changes), then vertical pass + centre pad + normalisation + store.
 *
 * One opa_pre_image per image.  All sizes in pixels, offsets as stated.  The caller keeps the table twice: on the host (read
 * here, for the checks and the launch geometry) and on the device (read by the kernels).
 *  mode 0 (Pillow's 8-bit BILINEAR resampler, the reference's default without OpenCV): x_table / y_table are the offsets, in
 *    int32 words into tables_dev, of the axis' coefficient table [1 + ksize][out_size]: row 0 the first source sample of every
 *    output sample, rows 1..ksize its weights with 22 fractional bits (non-negative, summing to ~2^22: the accumulator is
 *    int32, starts at 2^21, is shifted right by 22 and clamped to 0..255; the horizontal pass rounds to uint8 first, like
 *    Pillow).  An axis whose size does not change is copied and its table is not read.
 *  mode 1 (scipy.ndimage.zoom, order 1: --precise-rescaling): the axis table is i0[n], i1[n], outside[n] (int32) and, from the
 *    next even word on, w0[n], w1[n] (float64), n = out_size; ksize is 2.  The four products (v * wy) * wx are summed in double
 *    in scipy's order, zeroed where outside, clamped to 0..255 and rounded as floor(t + 0.5).  No intermediate is used.
 * Table offsets are multiples of 4 words.  Source indices from the tables are clamped to the frame by the kernels. */
typedef struct opa_pre_image {
    int64_t src_offset;       /* bytes from frames_dev to the frame: uint8 [h0, w0, 3], dense, any alignment          */
    int64_t mid_offset;       /* bytes from workspace_dev to the image's intermediate (mode 0, tw != w0 only): uint8
                               * [h0, pitch] with pitch = 3 * tw rounded up to 16; a multiple of 16                     */
    int32_t h0, w0;           /* frame size                                                                            */
    int32_t th, tw;           /* size after the rescale (equal to h0, w0: no rescale)                                  */
    int32_t top, left;        /* where the rescaled frame is placed on the canvas; the rest gets the fill colour       */
    int32_t x_table, x_ksize; /* horizontal coefficient table: offset in int32 words, taps per output sample           */
    int32_t y_table, y_ksize; /* vertical coefficient table                                                            */
} opa_pre_image;
size_t opa_pre_image_bytes(void);

/* Bytes of intermediate workspace a batch needs when its images' mid_offset are assigned in order, each region
 * h0 * pitch bytes rounded up to 256 (mode 1: 0).  0 with opa_last_error() set for a bad argument. */
size_t opa_preprocess_workspace_bytes(const opa_pre_image* images_host, int32_t batch, int32_t mode);

/* Queue the passes on `stream`.
 *  frames_dev     packed frames, 16-B aligned, frames_bytes a multiple of 16 (rows are fetched as aligned 16-B vectors)
 *  tables_dev     int32 [tables_words], 16-B aligned
 *  workspace_dev  16-B aligned, workspace_bytes >= opa_preprocess_workspace_bytes (may be NULL when that is 0)
 *  lut_dev        float32 [3][256]: the normalised value of every byte per channel (the caller forms it with the host
 *                 pipeline's own expression, (float32(v) / 255 - mean) / std, so the kernels divide nothing)
 *  out_dev        float32 [batch, 3, canvas_h, canvas_w], or with channels_last != 0 [batch, canvas_h, canvas_w, 3]
 *  fill_rgb       padding colour, r | g << 8 | b << 16 (the reference: 124, 116, 104)
 * Checked before anything is queued (OPA_ERR_INVALID_ARGUMENT, the text names the field): null pointers, alignment,
 * batch < 1, canvas sides < 1, h0 / w0 / th / tw < 1, a placement outside the canvas, ksize < 1, offsets outside their
 * buffers; a workspace that is too small is OPA_ERR_WORKSPACE.  Limits (OPA_ERR_INVALID_ARGUMENT beyond them): batch and
 * canvas_h at most 65535; h0 * w0 and h0 * tw below 2^30 per image (which also keeps the horizontal pass' grid,
 * h0 * ceil(tw / 256) workgroups per image, launchable); the source pixels 256 output columns of one row reach must fit
 * 64 KB of LDS (a horizontal reduction of up to ~80x). */
int opa_preprocess_u8(const opa_pre_image* images_host, const opa_pre_image* images_dev, int32_t batch,
                      const uint8_t* frames_dev, size_t frames_bytes, const int32_t* tables_dev, size_t tables_words,
                      uint8_t* workspace_dev, size_t workspace_bytes, const float* lut_dev, float* out_dev,
                      int32_t canvas_h, int32_t canvas_w, int32_t mode, int32_t channels_last, uint32_t fill_rgb,
                      void* stream);

/* ---- measurement -------------------------------------------------------- */
/* Per-kernel timing with HIP events on the launch stream (no reference
 * counterpart; bench.py's roofline leg uses it).  Between opa_profile_begin and
 * opa_profile_end every kernel/memset the library enqueues from THIS host thread
 * is followed by an event record; opa_profile_end synchronises the stream and
 * returns, per enqueued operation in order, its name (static string) and the
 * elapsed milliseconds since the previous event. */
int opa_profile_begin(void* stream);
int opa_profile_end(int32_t capacity, const char** names_out, float* ms_out, int32_t* n_out);

#ifdef __cplusplus
}
#endif
#endif  /* OPENPIFPAF_AMD_H_ */
