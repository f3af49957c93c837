/* tmc2hip.h -- C-ABI of the MI355X-native TMC2 patch-generation / image-generation hot path.
 *
 * This is the drop-in boundary.  The reference has no FFI around this path: the
 * seams are C++ member functions of PCCPatchSegmenter3 / PCCNormalsGenerator3 / PCCKdTree / PCCEncoder
 * / PCCMetrics.  Each entry point below names the reference member it replaces (file:line relative
 * to the reference tree); INTEGRATION.md shows the adaptor a maintainer adds at each call site.
 *
 * Conventions
 *   - plain C, POD only; every function returns 0 on success or a negative TMC2_E_* code and never
 *     throws or exits (the reference exit()s on fatal conditions, e.g. PCCPatch.cpp:242);
 *     tmc2_last_error() returns a human-readable message for the calling thread's last failure.
 *   - a tmc2_ctx is bound to ONE HIP device and owns one stream; it is not thread-safe, create one
 *     per host thread (the reference calls the segmenter from a tbb::parallel_for over frames,
 *     PCCEncoder.cpp:4729-4750 -- one ctx per in-flight frame).
 *   - a tmc2_frame holds the device-resident state of one point-cloud frame; stage functions chain
 *     on it without bouncing through the host.  Host arrays are AoS exactly like the reference
 *     containers: xyz = int16[n][3] (PCCPoint3D, PCCMath.h:450), rgb = uint8[n][3] (PCCColor3B :453),
 *     normals = double[n][3].
 *   - there is NO CPU fallback: without a HIP device tmc2_ctx_create fails with TMC2_E_NO_DEVICE.
 */
#ifndef TMC2HIP_H
#define TMC2HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TMC2_OK 0
#define TMC2_E_NO_DEVICE -1
#define TMC2_E_HIP -2
#define TMC2_E_INVALID -3
#define TMC2_E_UNSUPPORTED -4
#define TMC2_E_STATE -5
/* a host restatement (tmc2_host_metrics_compute) whose answer would depend on the k-d tree's visiting order, which it does not know */
#define TMC2_E_ORDER -6

typedef struct tmc2_ctx   tmc2_ctx;
typedef struct tmc2_frame tmc2_frame;

/* Flat mirror of the live fields of PCCPatchSegmenter3Parameters (PCCPatchSegmenter.h:48-100) as
 * filled by PCCEncoder::generateSegments (PCCEncoder.cpp:4672-4723).  Options the CTC lossy
 * conditions keep off are not representable; tmc2_segmenter_params_check() documents them.        */
typedef struct tmc2_segmenter_params {
  int32_t nnNormalEstimation;               /* 16  */
  int32_t normalOrientation;                /* 1 = PCC_NORMALS_GENERATOR_ORIENTATION_SPANNING_TREE */
  int32_t gridBasedRefineSegmentation;      /* 1   */
  int32_t maxNNCountRefineSegmentation;     /* 1024 */
  int32_t iterationCountRefineSegmentation; /* 10 / 50 longdress / 20 basketball */
  int32_t voxelDimensionRefineSegmentation; /* 4   */
  int32_t searchRadiusRefineSegmentation;   /* 192 */
  int32_t occupancyResolution;              /* 16  */
  int32_t enablePatchSplitting;             /* 1   */
  int32_t maxPatchSize;                     /* 1024 */
  int32_t quantizerSizeX;                   /* 1 << log2QuantizerSizeX = 16 */
  int32_t quantizerSizeY;                   /* 16  */
  int32_t minPointCountPerCCPatchSegmentation; /* 16 */
  int32_t maxNNCountPatchSegmentation;      /* 16  */
  int32_t surfaceThickness;                 /* 4   */
  int32_t mapCountMinus1;                   /* 1   */
  int32_t minLevel;                         /* 64  */
  int32_t maxAllowedDepth;                  /* (1 << geometryNominal2dBitdepth) - 1 = 255 */
  int32_t geometryBitDepth2D;               /* 8   */
  int32_t geometryBitDepth3D;               /* geometry3dCoordinatesBitdepth + 1 = 11 / 12 */
  double  maxAllowedDist2RawPointsDetection; /* 9 */
  double  maxAllowedDist2RawPointsSelection; /* 1 */
  double  lambdaRefineSegmentation;          /* 3 */
  double  weightNormal[3];                   /* PCCEncoder::calculateWeightNormal, see tmc2_weight_normal */
} tmc2_segmenter_params;

/* One patch record = the PCCPatch fields the hot path produces (PCCPatch.h:352-409).
 * depthOffset / occOffset index the frame's pools (see tmc2_frame_get_patches).                     */
typedef struct tmc2_patch {
  int32_t index, viewId;
  int32_t normalAxis, tangentAxis, bitangentAxis, projectionMode;
  int32_t u1, v1, d1;
  int32_t sizeU, sizeV, sizeD, sizeDPixel;
  int32_t sizeU0, sizeV0;
  int32_t size2DXInPixel, size2DYInPixel;
  int32_t d0Count, eomAndD1Count;
  int32_t u0, v0, patchOrientation; /* set by packing */
  int64_t depthOffset;
  int64_t occOffset;
} tmc2_patch;

/* ---- context ------------------------------------------------------------------------------- */
int         tmc2_ctx_create( int device, tmc2_ctx** out );
void        tmc2_ctx_destroy( tmc2_ctx* ctx );
const char* tmc2_last_error( void );
int         tmc2_ctx_synchronize( tmc2_ctx* ctx );
/* Page-locked host memory that every device of the node can DMA into (hipHostMalloc, portable): where a native front end lands
 * the finished canvases -- what the reference keeps in PCCVideo<T> frames for the video encoder (PCCVideo.h) -- so that the
 * copies out of HBM are plain DMA from each GPU over its own PCIe link (integration/tmc2_encode_gof.cpp).          */
int         tmc2_host_alloc( size_t bytes, void** out );
void        tmc2_host_free( void* p );
/* ... and the same for memory the caller already has (a shared-memory segment that several processes of the node map: every
 * rank of a one-process-per-GPU run lands its frames' canvases where the process that runs the video encoder reads them) */
int         tmc2_host_register( void* p, size_t bytes );
int         tmc2_host_unregister( void* p );
/* Limit on concurrently running host-resident steps (k-d tree builds of option KDTREE_HOST, the normal orientation's walk); 0 =
 * none.  Frames of a GOF run on separate host threads; the gate keeps the cache-hungry host steps at the core-complex count while
 * the GPU phases of the other frames proceed.  A gate is an object an encoder shares among ITS contexts (round 6: two encoders of
 * one process do not draw on one count): tmc2_host_gate_create, tmc2_ctx_set_host_gate( ctx, gate ) on each (gate NULL: back to the
 * default), tmc2_host_gate_destroy when the encoder is done (contexts that still hold it keep it alive).  A context without a gate
 * uses the process' default one, whose limit tmc2_set_host_parallelism presets -- the last of the old process-wide setters, kept
 * for callers that have a single encoder.                                                                              */
typedef struct tmc2_host_gate tmc2_host_gate;
int         tmc2_host_gate_create( int maxConcurrentHostSteps, tmc2_host_gate** out );
void        tmc2_host_gate_destroy( tmc2_host_gate* gate );
int         tmc2_ctx_set_host_gate( tmc2_ctx* ctx, tmc2_host_gate* gate );
void        tmc2_set_host_parallelism( int maxConcurrentHostSteps );
/* Per-context options: everything that tunes or cross-checks the path is a property of ONE context -- no process-global state, and
 * the library does not look at the environment while it runs.  key = the knob's name (DESIGN.md section 5 lists them):
 * "REFINE_OVERLAP" (0 / 1, below), "KDTREE_HOST" (0 / 1 / 2, below), "UF_PRECHECK" / "UF_SCOPE" / "UF_CHECK" (the union passes'
 * conservative forms and debug invariants), "KD_HUGEMAX" / "KD_DECIDE" (forms of the device tree build),
 * "REFINE_*" (forms and grids of the refinement), "METRICS_K", "ORIENT_*"; a "TMC2_" prefix is accepted and dropped.  When a
 * context is created its options start as the TMC2_* variables of the process environment (read once, there); value NULL
 * unsets an option.  None of them ever changes a result.  Options may be set from any thread while frames of the context are
 * in flight (a mutex guards the table; a stage reads an option when it starts).  tmc2_ctx_get_option returns a pointer to a COPY
 * held in one string reserved for it per calling thread, valid until that thread's next tmc2_ctx_get_option call -- never a
 * pointer into the table; NULL if the option is unset.
 * "POOL_POISON" (for tests; unset by default): a byte 0 .. 255, decimal or 0x.. -- anything else is refused with TMC2_E_INVALID, by
 * tmc2_ctx_set_option and, for a TMC2_POOL_POISON of the environment, by tmc2_ctx_create.  While it is set, every block the
 * context's pool hands out (a recycled block, a piece of reserved memory, a fresh allocation) is filled with that byte over its
 * whole size class, on the context's stream, and the fill is waited for: slow, and a stage that reads a word it has not written
 * computes from the poison instead of from what the block's last owner left.  It changes no result -- that is what it tests.
 * Memory that does not come from the pool is not filled: tmc2_ctx_device_alloc, a buffer allocated with no context entered,
 * page-locked host staging; nor is a buffer that keeps its block from one call to the next.  "POOL_POISON_STAGE" = a stage name
 * (tmc2_ctx_stage_name) narrows the fill to the blocks acquired while a stage of that name is open (set both between stages).
 * tmc2_option_check: what tmc2_ctx_set_option would answer for this key and value, without a context (host only).       */
int         tmc2_ctx_set_option( tmc2_ctx* ctx, const char* key, const char* value );
const char* tmc2_ctx_get_option( tmc2_ctx* ctx, const char* key );
int         tmc2_option_check( const char* key, const char* value );
/* Reserve, at context creation time, the device memory the frames of a sequence will need (upper bounds of the sequence: points
 * per frame, voxelDimensionRefineSegmentation, geometry3dCoordinatesBitdepth + 1, the largest canvas).  The reference sizes its
 * containers per frame as it goes (std::vector growth inside PCCPatchSegmenter3::compute / PCCEncoder::generateGeometryVideo); here
 * every temporary comes from the context's caching pool, whose FIRST use of a size is a hipMalloc -- a device-wide synchronisation
 * under all frames in flight: the first GOFs of a process ran at half speed.  With the reservation the pool carves from memory it
 * already holds.  Optional; a frame that needs more than was reserved still works (hipMalloc).                        */
int         tmc2_ctx_reserve( tmc2_ctx* ctx, uint64_t maxPoints, int voxelDimRefine, int bits3d, int maxCanvasWidth, int maxCanvasHeight );
int         tmc2_ctx_pool_stats( tmc2_ctx* ctx, uint64_t* bytesHeld, uint64_t* mallocCalls, double* mallocMs, uint64_t* carvedBlocks );
/* Device staging for a host that exchanges small records between the ranks of a sharded GOF itself (libtmc2gof.so over RCCL,
 * include/tmc2gof.h: the collectives need device buffers and the stream they become ready on): memory of the context's device,
 * copies ordered on the context's stream (download waits for it), the stream (a hipStream_t) and the device ordinal.      */
int         tmc2_ctx_device_alloc( tmc2_ctx* ctx, size_t bytes, void** out );
int         tmc2_ctx_device_free( tmc2_ctx* ctx, void* p );
int         tmc2_ctx_upload( tmc2_ctx* ctx, void* deviceDst, const void* hostSrc, size_t bytes );
int         tmc2_ctx_download( tmc2_ctx* ctx, void* hostDst, const void* deviceSrc, size_t bytes );
void*       tmc2_ctx_stream( tmc2_ctx* ctx );
int         tmc2_ctx_device( tmc2_ctx* ctx );
int         tmc2_ctx_make_current( tmc2_ctx* ctx );
/* per-stage GPU time of the last frame operation, milliseconds (hipEvent); name list via index */
int         tmc2_ctx_stage_count( tmc2_ctx* ctx );
const char* tmc2_ctx_stage_name( tmc2_ctx* ctx, int i );
double      tmc2_ctx_stage_ms( tmc2_ctx* ctx, int i );
long        tmc2_ctx_stage_calls( tmc2_ctx* ctx, int i );
void        tmc2_ctx_stage_reset( tmc2_ctx* ctx );
void        tmc2_ctx_set_timing( tmc2_ctx* ctx, int enabled ); /* hipEvent timing of stages on/off (default on) */

/* ---- frame: upload + PCCKdTree ------------------------------------------------------------- */
/* replaces: PCCKdTree::PCCKdTree(const PCCPointSet3&) / init  (PccLibCommon/source/PCCKdTree.cpp:44-59).
 * Copies the points to HBM; the nanoflann-identical k-d tree (leaf size 10) is built on first use.   */
int  tmc2_frame_create( tmc2_ctx* ctx, const int16_t* xyz, const uint8_t* rgb, uint64_t n, tmc2_frame** out );
void tmc2_frame_destroy( tmc2_frame* f );
/* the tree is built (host) and uploaded on first use; this forces it (PCCKdTree::init, PCCKdTree.cpp:56-59) */
int  tmc2_kdtree_build( tmc2_frame* f );
/* where PCCKdTree::init runs: option "KDTREE_HOST" of the frame's context; this call presets what contexts WITHOUT the option do
 * (rounds 1-4's process-wide switch).  0 (default): on the device, lowest latency for a frame on its own;
 * 1: on the host (same algorithm, same tree) -- with many frames in flight and idle host cores this leaves the
 * GPU to the stages only it can run; 2: adaptive -- on the host while one of the host slots
 * (tmc2_set_host_parallelism) is free at that moment, else on the device.  Both builders are exact; the choice
 * never changes a result.                                                                                   */
void tmc2_set_kdtree_placement( int mode );
/* option "REFINE_OVERLAP" of the frame's context (this call presets what contexts WITHOUT the option do):
 * tmc2_segmenter_compute queues the geometry of the refinement (S5: voxels, neighbourhood rows -- it needs the
 * points only) before the host-resident walk of the normal orientation (S3) and builds it while the host walks.  Shortens a
 * frame's chain (few frames in flight: one rank of a many-GPU run); with the chip full of other frames it only competes with
 * them -- off by default.  The same setting makes the two kernels of a refinement sweep take the grids that are fastest with
 * the GPU to themselves (twice the workgroups: idle waves are in nobody's way then).  Never changes a result.        */
void tmc2_set_refine_overlap( int on );
/* inspection: the permutation nanoflann's build leaves in vind (tree order -> point index), uint32[n], and the
 * number of tree levels; the search order under distance ties is a function of exactly this permutation */
int  tmc2_frame_get_kdtree_order( tmc2_frame* f, uint32_t* perm, int32_t* depth );
uint64_t tmc2_frame_point_count( const tmc2_frame* f );
/* drop every derived result (tree, adjacency, normals, partition, patches, canvases); the points stay in HBM */
int  tmc2_frame_reset( tmc2_frame* f );

/* replaces: PCCKdTree::search (PCCKdTree.cpp:61-66) for a batch of queries against the frame's tree.
 * idx = uint32[nq][k] in nanoflann result order; dist2 = uint32[nq][k] squared distances or NULL.   */
int tmc2_kdtree_search( tmc2_frame* f, const int16_t* queries, uint64_t nq, int k, uint32_t* idx, uint32_t* dist2 );
/* replaces: PCCKdTree::search for result counts beyond the per-lane kernel's (PCCPatchSegmenter3::computeAdjacencyInfo with
 * maxNNCountRefineSegmentation, PCCPatchSegmenter.cpp:267-291).  queries NULL: the frame's own points (row i = point i; nq is then
 * the frame's point count).  idx uint32[nq][k]: the k results of nanoflann's search as a SET -- the first k points under the key
 * (squared distance, position in the query's depth-first visiting order); the order inside a row is unspecified.  Always the
 * wave-per-query kernel (csrc/knn_wide.hip), whatever k.  TMC2_E_INVALID for k < 1 or k > the cloud, TMC2_E_UNSUPPORTED for
 * k > 1024 and for a coordinate below -4096 (squared distances are 32-bit).                                                  */
int tmc2_kdtree_search_wide( tmc2_frame* f, const int16_t* queries, uint64_t nq, int k, uint32_t* idx );

/* ---- PCCNormalsGenerator3 ------------------------------------------------------------------- */
/* replaces: PCCNormalsGenerator3::computeNormals (PccLibEncoder/source/PCCNormalsGenerator.cpp:158-185)
 * and, sharing its k-NN lists, PCCPatchSegmenter3::computeAdjacencyInfo (PCCPatchSegmenter.cpp:267-291). */
int tmc2_normals_compute_normals( tmc2_frame* f, int k );
/* replaces: PCCNormalsGenerator3::orientNormals, SPANNING_TREE branch (PCCNormalsGenerator.cpp:198-242).  */
int tmc2_normals_orient( tmc2_frame* f );
/* replaces: PCCNormalsGenerator3::compute (PCCNormalsGenerator.cpp:61-70) = both of the above.          */
int tmc2_normals_compute( tmc2_frame* f, int k, int orientation );
int tmc2_frame_get_normals( tmc2_frame* f, double* normals /* [n][3] */ );
int tmc2_frame_set_normals( tmc2_frame* f, const double* normals );
int tmc2_frame_get_adjacency( tmc2_frame* f, uint32_t* adj /* [n][k] */ );

/* ---- PCCEncoder::calculateWeightNormal (PCCEncoder.cpp:3569-3626) ---------------------------- */
int tmc2_weight_normal( tmc2_frame* f, int geometryBitDepth3D, double minWeightEPP, double weight[3] );

/* ---- PCCPatchSegmenter3 stages --------------------------------------------------------------- */
/* replaces: PCCPatchSegmenter3::initialSegmentation (PCCPatchSegmenter.cpp:226-265), 6 planes.        */
int tmc2_segmenter_initial_segmentation( tmc2_frame* f, const double weight[3] );
/* replaces: PCCPatchSegmenter3::refineSegmentationGridBased (PCCPatchSegmenter.cpp:1386-1561).       */
int tmc2_segmenter_refine_grid_based( tmc2_frame* f, int maxNNCount, double lambda, int iterationCount,
                                      int voxDim, int searchRadius );
/* replaces: PCCPatchSegmenter3::refineSegmentation (PCCPatchSegmenter.cpp:1322-1384) on the frame's normals and partition: the
 * maxNNCount nearest neighbours of every point (tmc2_kdtree_search_wide's set), then iterationCount Jacobi rounds; a round that
 * changes no point ends the loop on the device (later rounds are no-ops in the reference too).  The neighbourhoods are scratch of
 * the context, n x maxNNCount x 4 bytes, grown on demand and NOT part of tmc2_ctx_reserve; the frame's k = 16 adjacency is left
 * alone.  TMC2_E_UNSUPPORTED, with the frame left as it was, for maxNNCount outside 1..1024 or above the cloud's point count (the
 * reference pads such rows with point 0), a negative iterationCount, a negative or NaN lambda.                                */
int tmc2_segmenter_refine( tmc2_frame* f, int maxNNCount, double lambda, int iterationCount );
int tmc2_frame_get_partition( tmc2_frame* f, uint32_t* partition /* [n] */ );
int tmc2_frame_set_partition( tmc2_frame* f, const uint32_t* partition );
/* replaces: PCCPatchSegmenter3::segmentPatches (PCCPatchSegmenter.cpp:542-1320).                      */
int tmc2_segmenter_segment_patches( tmc2_frame* f, const tmc2_segmenter_params* p );
/* replaces: PCCPatchSegmenter3::compute (PCCPatchSegmenter.cpp:53-150) = S1..S9 end to end.           */
int tmc2_segmenter_compute( tmc2_frame* f, const tmc2_segmenter_params* p );
/* TMC2_OK, or TMC2_E_UNSUPPORTED with a message "params: ..." naming the field.  Refused: options the path does not implement
 * (k-NN counts other than 16, normalOrientation other than 0 / 1, gridBasedRefineSegmentation off, occupancyResolution other
 * than 16, mapCountMinus1 other than 1); values no stage can compute (minLevel < 1 or beyond the geometry bit depth, bit
 * depths outside 1..16, negative surfaceThickness / minPointCount / quantizer sizes, maxPatchSize < 1, raw-point thresholds
 * outside 0..27, maxNNCountRefineSegmentation < 1, negative lambda, a voxel size that is no power of two >= 2, a search
 * radius below one voxel or whose ball the LDS tile does not hold: radius >> log2(voxel) > 97); and
 * maxAllowedDepth < surfaceThickness + minLevel - 1, where the reference's own loop over the raw points never ends.
 * Two inputs on which that loop never ends depend on the cloud and cannot be refused here: tmc2_segmenter_segment_patches /
 * tmc2_segmenter_compute end with TMC2_E_UNSUPPORTED when patch splitting keeps no point of a component, or when a round
 * takes no point off the raw list.                                                                                         */
int tmc2_segmenter_params_check( const tmc2_segmenter_params* p );
/* replaces: PCCPatchSegmenter3::compute with gridBasedSegmentation_ (PCCPatchSegmenter.cpp:78-149) -- the reference's fast mode
 * (m56857): the cloud is voxelised (convertPointsToVoxels :152-181), tree, normals, orientation, initial segmentation and
 * refinement run on the voxel cloud with p's values, partition and normals are copied back to the points (applyVoxelsDataToPoints
 * :183-215); tree, k = 16 adjacency and segmentPatches then run on the full cloud.  p as for the plain call -- the reference's fast
 * mode presets maxNNCountRefineSegmentation 384, iterationCountRefineSegmentation 5, voxelDimensionRefineSegmentation 2,
 * searchRadiusRefineSegmentation 128 (PCCEncoderParameters.cpp:64-67), which apply to the voxel coordinates; weightNormal is that
 * of the original cloud.  Afterwards the frame is what the plain call leaves: normals (copies of the voxels', bit for bit),
 * partition, adjacency and tree of the full cloud, patches, pools.  TMC2_E_UNSUPPORTED, with the frame left as it was, for a
 * voxelDimensionGridBasedSegmentation other than 2, 4 or 8, a voxel coordinate that does not fit geometryBitDepth3D bits (the
 * reference's voxel names would collide; negative coordinates included) and a voxel cloud of fewer than 16 points.          */
int tmc2_segmenter_compute_grid_based( tmc2_frame* f, const tmc2_segmenter_params* p, int voxelDimensionGridBasedSegmentation );
/* replaces: PCCPatchSegmenter3::compute with gridBasedRefineSegmentation_ off (:126-131).  p->gridBasedRefineSegmentation must be
 * 0; voxelDimensionGridBasedSegmentation 0: the plain chain; 2, 4, 8: the fast mode with this refinement on the voxel cloud.
 * tmc2_segmenter_params_check's rules apply with the one on gridBasedRefineSegmentation reversed; voxelDimensionRefineSegmentation
 * and searchRadiusRefineSegmentation are not read; maxNNCountRefineSegmentation must lie in 1..1024 (the reference's default with
 * the flag off is 256, with 100 iterations) and iterationCountRefineSegmentation must be >= 0.  A cloud, or a voxel cloud, of
 * fewer than maxNNCountRefineSegmentation points is TMC2_E_UNSUPPORTED by name, with the frame left as it was, as are the
 * refusals of tmc2_segmenter_compute_grid_based.  The neighbourhoods are context scratch outside tmc2_ctx_reserve
 * (tmc2_segmenter_refine).                                                                                               */
int tmc2_segmenter_compute_knn_refine( tmc2_frame* f, const tmc2_segmenter_params* p, int voxelDimensionGridBasedSegmentation );
/* replaces: PCCPatchSegmenter3::convertPointsToVoxels (PCCPatchSegmenter.cpp:152-181) alone, on a host cloud, on the device: the
 * voxel of a point is ( ( x + voxDim / 2 ) >> log2 voxDim, .. ) -- rounding, not floor; voxelXyz int16[n][3] takes the voxels in
 * the order of their first point (the first *voxelCount rows are written), voxelOfPoint uint32[n] the rank of every point's voxel
 * in that list.  Same status as the tmc2_selftest_ family: the new code on its own.  Refusals as above (bits = geometryBitDepth3D). */
int tmc2_segmenter_convert_points_to_voxels( tmc2_ctx* ctx, const int16_t* xyz, uint64_t n, int voxDim, int bits, int16_t* voxelXyz,
                                             uint64_t* voxelCount, uint32_t* voxelOfPoint );

/* patch list of the frame (after segment_patches / compute) */
int tmc2_frame_patch_count( tmc2_frame* f );
int tmc2_frame_patch_pool_sizes( tmc2_frame* f, int64_t* depthCount, int64_t* occCount );
int tmc2_frame_get_patches( tmc2_frame* f, tmc2_patch* patches, int16_t* depth0, int16_t* depth1, uint8_t* occupancy );

/* ---- PCCEncoder image generation, phase A (all-intra packing) ---------------------------------- */
/* replaces: PCCEncoder::packFlexible (PccLibEncoder/source/PCCEncoder.cpp:2306-2449) for one frame, as called by
 * PCCEncoder::placeSegments (:4762-4835) with constrainedPack=0, packingStrategy=1, two orientations.
 * Sorts the patch list (PCCPatch::gt), assigns u0/v0/patchOrientation, returns the frame's canvas height.  */
int tmc2_encoder_pack_flexible( tmc2_frame* f, int presetWidth, int numTilesHor, double tileHeightToWidthRatio,
                                int32_t* height );
/* replaces: PCCEncoder::spatialConsistencyPackFlexible (PccLibEncoder/source/PCCEncoder.cpp:1183-1412) for one frame, as called
 * by placeSegments (:4790-4795) for frames after the first when constrainedPack = 1 (the program default and the CTC
 * low-delay condition; globalPatchAllocation 0), packingStrategy = 1, two orientations: patches are matched to those of
 * `previous` (same view, bounding-box IoU > 0.2, pcc::computeIOU PCCPatchSegmenter.cpp:1563), matched ones go first,
 * in the previous frame's order and if possible at the previous position.  `previous` must be packed already.       */
int tmc2_encoder_pack_spatial_consistency( tmc2_frame* f, tmc2_frame* previous, int presetWidth, int numTilesHor,
                                           double tileHeightToWidthRatio, int32_t* height );
/* the tile size the packers left behind (what resizeTileGeometryVideo / resizeGeometryVideo look at): packFlexible keeps the
 * preset width, spatialConsistencyPackFlexible and the global patch allocation set the width of the canvas they packed on */
int tmc2_frame_get_packed_size( tmc2_frame* f, int32_t* width, int32_t* height );
/* per list position: the position of the matched patch in the previous frame's list (PCCPatch::getBestMatchIdx), -1 = none
 * (all -1 after tmc2_encoder_pack_flexible) */
int tmc2_frame_get_patch_matches( tmc2_frame* f, int32_t* matches );
/* replaces: PCCEncoder::performDataAdaptiveGPAMethod (PccLibEncoder/source/PCCEncoder.cpp:6821-6971) with the members it
 * drives (generateGlobalPatches :7022, unionPatchGenerationAndPacking :7059, packingFirstFrame :7228, performGPAPacking
 * :7531, updatePatchInformation :7366), as placeSegments runs it after the per-frame packing chain when constrainedPack = 1
 * and globalPatchAllocation = 1 (the CTC random-access condition).  frames[0..count): the frames of the GOF in order, each
 * packed (tmc2_encoder_pack_flexible for the first, tmc2_encoder_pack_spatial_consistency for the others).  Patches tracked
 * across the frames of a sub-context take the block size of the union of their track and one common position; every
 * frame's list is reordered (tracked patches first, aligned across frames), patch.index becomes the list position,
 * sizeU0 / sizeV0 / u0 / v0 / patchOrientation, the matches and the block-occupancy pool are rewritten; afterwards
 * tmc2_frame_get_patches returns the records in list order and tmc2_frame_get_patch_order the identity.
 * widths / heights (int32[count], may be NULL): the tile size of every frame for tmc2_encoder_canvas_size.          */
int tmc2_encoder_global_patch_allocation( tmc2_frame** frames, int count, int minimumImageWidth, int minimumImageHeight,
                                          int32_t* widths, int32_t* heights );
/* A frame sharded onto another rank takes part in the inter-frame packers through its patch RECORDS: they travel to the
 * rank that runs the chain (tmc2_host_pack_flexible / _spatial_consistency / _global_patch_allocation on plain records,
 * "gather to rank 0 of the per-frame patch table before packing"), the packed list comes back and is installed
 * here -- what PCCEncoder::placeSegments leaves in the frame's PCCFrameContext (PCCEncoder.cpp:4790-4840).
 * list[count]: the frame's patches in LIST order with u0 / v0 / patchOrientation (and, after the global patch allocation,
 * rewritten index / sizeU0 / sizeV0) and occOffset into occupancy[occupancyBytes] (pool in list order); depthOffset must
 * still point into this frame's own depth pools.  matches: int32[count] or NULL (none).  packedWidth / packedHeight: the
 * tile size the packers left.  Afterwards the frame is in the state tmc2_encoder_global_patch_allocation leaves.      */
int tmc2_frame_set_packing( tmc2_frame* f, const tmc2_patch* list, int count, const int32_t* matches, const uint8_t* occupancy,
                            int64_t occupancyBytes, int packedWidth, int packedHeight );
/* packing order of the frame: order[listPosition] = patch index (the reference reorders the list itself) */
int tmc2_frame_get_patch_order( tmc2_frame* f, int32_t* order );
/* replaces: resizeTileGeometryVideo + resizeGeometryVideo (PCCEncoder.cpp:5593-5632, 5546-5591): common GOF canvas */
int tmc2_encoder_canvas_size( const int32_t* frameHeights, int frames, int tileWidth, int minimumImageWidth,
                              int minimumImageHeight, int32_t* width, int32_t* height );
/* replaces, for one frame: generateOccupancyMap (:3767-3784), generateOccupancyMapVideo (:806-861),
 * PCCCodec::generateBlockToPatchFromOccupancyMapVideo (PccLibCommon/source/PCCCodec.cpp:1736-1775),
 * generateGeometryVideo -> generateIntraImage (:3929-3992) + dilate3DPadding (:5951-6130, geometryPadding=0)
 * + dilateGroupGeometryVideo (:3717-3739).                                                              */
int tmc2_encoder_generate_geometry_images( tmc2_frame* f, int width, int height, int occupancyPrecision );
/* canvases of the frame; any pointer may be NULL.  occupancy u8[W*H], occVideo u8[(W/p)*(H/p)],
 * blockToPatch u32[(W/16)*(H/16)] (list position + 1), geometry D0 / D1 luma u16[W*H] (chroma planes are zero) */
int tmc2_frame_get_geometry_images( tmc2_frame* f, uint8_t* occupancy, uint8_t* occVideo, uint32_t* blockToPatch,
                                    uint16_t* geometryD0, uint16_t* geometryD1 );
/* ---- PCCEncoder image generation, phase B (after the geometry video has been coded and decoded) -------- */
/* replaces, for one frame: PCCCodec::generatePointCloud (PccLibCommon/source/PCCCodec.cpp:519-980, lossy CTC branch),
 * PCCPointSet3::transferColors source -> reconstruction (PccLibCommon/source/PCCPointSet.cpp:807-1124, CTC settings),
 * presmoothPointCloudColor (PCCEncoder.cpp:6593-6655, a no-op in the reference build), generateAttributeVideo
 * (:6736-6794), dilateSmoothedPushPull (:6542-6591) and the attribute group dilation (encode() :380-402).
 * Works on the frame's resident occupancy / geometry canvases (decoded == generated when the codec is lossless;
 * upload decoded planes with tmc2_frame_set_decoded_geometry first when it is not).                         */
int     tmc2_encoder_generate_attribute_images( tmc2_frame* f );
/* replaces: PCCPointSet3::transferColors (PccLibCommon/source/PCCPointSet.cpp:807-1124) alone, on two host clouds, with the
 * arguments PCCEncoder::generateAttributeVideo passes under the CTC (PCCEncoder.cpp:6679-6697); tgtRgb = uint8[m][3]      */
int     tmc2_transfer_colors( tmc2_ctx* ctx, const int16_t* srcXyz, const uint8_t* srcRgb, uint64_t n, const int16_t* tgtXyz,
                              uint64_t m, uint8_t* tgtRgb );
/* The two entries above over the arguments of PCCPointSet3::transferColors, in its order -- the sixteen encoder options that
 * PCCEncoder::generateAttributeVideo hands over (PCCEncoder.cpp:6679-6697; defaults PCCEncoderParameters.cpp:96-110).
 * tmc2_color_transfer_params_default fills the CTC point, what the entries above compute: 0, 0, 8, 1, 1, 1, 1, 1, 4, 4, 1000,
 * 1000, 1000, 1000, 0, 10 -- with it the _ex entries run what the entries above run.
 * As the reference reads them: a threshold of 512 or more is none; the geometry threshold never drops the first forward result
 * but may drop every backward candidate (the target then keeps its forward colour); the pairwise colour maximum starts at
 * DBL_MIN, so a colour threshold of 0 always leaves the nearest colour alone; without the skip flag an identical point is
 * averaged with weight 1 / distOffset; a single remaining candidate counts unweighted; the outlier pass (weighted means only)
 * compares the dropped count with the shrunk length in both directions; the best-colour search visits the clipped cube
 * (2 searchRange + 1)^3 in lexicographic order and keeps the first strict minimum.
 * tmc2_color_transfer_params_check needs no device: TMC2_OK, TMC2_E_INVALID for NULL, or TMC2_E_UNSUPPORTED with the field named
 * in tmc2_last_error -- a neighbour count outside 1..32, searchRange outside 0..8, a distOffset that is not > 0, a negative or NaN
 * threshold or thresholdColorOutlierDist.  The entries refuse these, and a neighbour count above the searched cloud's size
 * (numNeighborsColorTransferFwd against the source, ..Bwd against the target), before the frame changes: the frame entry holds a
 * backward count above 1 against the size of the reconstruction it is about to make by counting the tiles first (one launch and a
 * scan that the CTC point does not pay), so a refused call leaves the previous reconstruction, colours and images in place.  A
 * source of more than 2^26 - 1 points is refused off the CTC point (backward entries are numbered source * K + rank in 32 bits).
 * No search asks for more results than its tree holds: a count between two search widths (1, 4, 8, 16, 32) runs the next wider
 * search and reads its first K; where that width is above the cloud's size the search runs at K itself.                     */
typedef struct tmc2_color_transfer_params {
  int32_t searchRange;
  int32_t losslessAttribute;
  int32_t numNeighborsColorTransferFwd, numNeighborsColorTransferBwd;
  int32_t useDistWeightedAverageFwd, useDistWeightedAverageBwd;
  int32_t skipAvgIfIdenticalSourcePointPresentFwd, skipAvgIfIdenticalSourcePointPresentBwd;
  double  distOffsetFwd, distOffsetBwd;
  double  maxGeometryDist2Fwd, maxGeometryDist2Bwd;
  double  maxColorDist2Fwd, maxColorDist2Bwd;
  int32_t excludeColorOutlier;
  double  thresholdColorOutlierDist;
} tmc2_color_transfer_params;
void tmc2_color_transfer_params_default( tmc2_color_transfer_params* params );
int  tmc2_color_transfer_params_check( const tmc2_color_transfer_params* params );
int  tmc2_transfer_colors_ex( tmc2_ctx* ctx, const int16_t* srcXyz, const uint8_t* srcRgb, uint64_t n, const int16_t* tgtXyz,
                              uint64_t m, const tmc2_color_transfer_params* params, uint8_t* tgtRgb );
int  tmc2_encoder_generate_attribute_images_ex( tmc2_frame* f, const tmc2_color_transfer_params* params );
int64_t tmc2_frame_recon_count( tmc2_frame* f );
/* reconstruction: xyz int16[M][3], rgb uint8[M][3], pointToPixel uint32[M][3] = (x, y, layer); any may be NULL */
int     tmc2_frame_get_reconstruction( tmc2_frame* f, int16_t* xyz, uint8_t* rgb, uint32_t* pointToPixel );
/* attribute images: uint8[2 maps][3 channels][H][W] (the reference holds the same values in uint16 planes) */
int     tmc2_frame_get_attribute_images( tmc2_frame* f, uint8_t* attribute );
/* replace the resident occupancy video / geometry planes by decoded ones (uint8[(W/p)*(H/p)], uint16[2][H][W]) */
int     tmc2_frame_set_decoded_geometry( tmc2_frame* f, const uint8_t* occVideo, const uint16_t* geometry );

/* device addresses of the frame's canvases (valid until the next generate call / frame destroy), for
 * zero-copy hand-off to a collective (RCCL gather of finished frames) or to a device-side consumer       */
int tmc2_frame_device_images( tmc2_frame* f, void** occupancy, void** occVideo, void** blockToPatch, void** geometry );
int tmc2_frame_device_attribute( tmc2_frame* f, void** attribute );

/* ---- colour-space conversion around the attribute video codec (PCCVideoEncoder::compress) -------------------------- */
/* replaces: PCCInternalColorConverter<T>::convert( "RGB444ToYUV420_8_<f>" ) (PccLibColorConverter/source/
 * PCCInternalColorConverter.cpp:355-378 -> convertRGB44ToYUV420 :406-424), which PCCVideoEncoder::compress
 * (PccLibEncoder/source/PCCVideoEncoder.cpp:353) runs on the attribute video before the codec when no external converter is
 * configured.  rgb: uint8 [3][H][W] (R, G, B planes); yuv420: one I420 frame, Y [H][W] then U, V [H/2][W/2].  Only the
 * reference's default filter (4 = DF_GS) is built; others return TMC2_E_UNSUPPORTED.                                 */
int tmc2_color_convert_rgb444_to_yuv420( tmc2_ctx* ctx, const uint8_t* rgb, int width, int height, int downsamplingFilter,
                                         uint8_t* yuv420 );
/* replaces: convert( "YUV420ToYUV444_8_<f>" ) (-> convertYUV420ToYUV444 :462-482) on the decoded video (PCCVideoEncoder.cpp:413;
 * the decoder does the same): 8-bit I420 frame -> uint16 [3][H][W], 16-bit 4:4:4.  Only filter 0 (UF_F0, the default). */
int tmc2_color_convert_yuv420_to_yuv444( tmc2_ctx* ctx, const uint8_t* yuv420, int width, int height, int upsamplingFilter,
                                         uint16_t* yuv444 );
/* the same two steps on a frame, without moving the source through the host: the resident attribute canvases as the two
 * I420 frames the attribute video encoder reads (yuv420: [2 maps] x I420 frame), and the two decoded I420 frames as the
 * 16-bit 4:4:4 planes that tmc2_codec_color_point_cloud( f, NULL ) then reads on the device                          */
int tmc2_encoder_attribute_to_yuv420( tmc2_frame* f, int downsamplingFilter, uint8_t* yuv420 );
int tmc2_codec_set_decoded_attribute_yuv420( tmc2_frame* f, const uint8_t* yuv420, int upsamplingFilter );
int tmc2_frame_get_decoded_attribute( tmc2_frame* f, uint16_t* planes ); /* uint16 [2][3][H][W] */

/* ---- decoder side: reconstruction from what the bitstream carries --------------------------------------------------- */
/* replaces what PCCDecoder::decode does per frame before the reconstruction (PccLibDecoder/source/PCCDecoder.cpp:333-349:
 * generateOccupancyMap, generateBlockToPatchFromOccupancyMapVideo -- PCCCodec.cpp:1736-1775): a frame WITHOUT a source
 * cloud, made of the decoded patch records in list order (u0, v0, sizeU0, sizeV0, patchOrientation, u1, v1, d1, the three
 * axes and projectionMode are used), the decoded occupancy video (uint8 [(H/p)][(W/p)]) and the two decoded geometry
 * maps (uint16 [2][H][W]).  Continue with tmc2_codec_generate_point_cloud and the tmc2_codec_* tail.                 */
int tmc2_decoder_frame_create( tmc2_ctx* ctx, const tmc2_patch* patches, int count, int width, int height, int occupancyPrecision,
                               const uint8_t* occVideo, const uint16_t* geometry, tmc2_frame** out );
/* replaces: PCCCodec::generatePointCloud (PccLibCommon/source/PCCCodec.cpp:519-980) alone -- the reconstruction from the
 * resident canvases without the encoder's colour transfer / attribute images (tmc2_encoder_generate_attribute_images runs it
 * as its first step).  tmc2_frame_get_reconstruction( f, xyz, NULL, pointToPixel ) returns the points.             */
int tmc2_codec_generate_point_cloud( tmc2_frame* f );
/* replaces: PCCCodec::generatePointCloud with pbfEnableFlag_ (PCCCodec.cpp:543-556, :664-669, :811) -- what the encoder
 * (PCCEncoder.cpp:556-560) and the decoder (PCCDecoder.cpp:333, from the occupancy-synthesis SEI) run instead when the stream
 * asks for occupancy synthesis: PatchBlockFiltering::patchBorderFiltering (PccLibCommon/source/PCCPatch.cpp:950-976, with
 * PCCPatch::setLocalData :797, generateBorderPoints3D :851, filtering :871) filters the occupancy of every patch at full
 * resolution against the border points of the patches next to it in 3-D, the reconstruction takes the filtered maps for its
 * occupancy test, and every point gets its boundary type (0 / 1) from PCCPatch::isBorder (:841) -- not from
 * identifyBoundaryPoints.  thresholdLossyOM: an occupancy-video sample counts as occupied above it (0 under the CTC);
 * passesCount / filterSize / log2Threshold: pbfPassesCount_, pbfFilterSize_, pbfLog2Threshold_.  Points, their order and
 * pointToPixel are those of tmc2_codec_generate_point_cloud on the filtered occupancy.  On such a frame
 * tmc2_codec_smooth_point_cloud_postprocess starts from the filter's flags, tmc2_codec_identify_boundary_points restores them,
 * and the colour transfer onto the moved points is not run (PCCEncoder.cpp:653, PCCDecoder.cpp:412);
 * tmc2_codec_generate_point_cloud returns the frame to the plain rule.  TMC2_E_UNSUPPORTED, naming the parameter, for precision
 * 16, a parameter outside 1 .. 127, filterSize + filterSize / 2 above the ring of the padded maps (8 pixels, 16 at precision 8)
 * and more than 65535 patches.  Where the filter removes every pixel the call succeeds as the reference does: the frame has its
 * maps and a reconstruction of no points, which the getters return as empty arrays and the tail's stages refuse by name
 * (TMC2_E_STATE).                                                                                                      */
int tmc2_codec_generate_point_cloud_pbf( tmc2_frame* f, int thresholdLossyOM, int passesCount, int filterSize, int log2Threshold );
/* what the filter left, for every patch in list order back to back: the interior sizeU0*16 x sizeV0*16 of
 * PCCPatch::getOccupancyMap( u, v ) and of PCCPatch::isBorder( u, v ), one byte per pixel, rows of v.  *pixels: their number. */
int tmc2_frame_patch_border_filtering_size( tmc2_frame* f, int64_t* pixels );
int tmc2_frame_get_patch_border_filtering( tmc2_frame* f, uint8_t* occupancy, uint8_t* border );

/* ---- post-reconstruction tail (PCCEncoder::encode :571-719, PCCDecoder::decode :330-470) -------------------- */
/* All of these work on the reconstruction left by tmc2_encoder_generate_attribute_images (PCCCodec::generatePointCloud on
 * the resident, or decoded, occupancy / geometry canvases).  CTC settings: two maps in one stream, lossy attributes,
 * flagGeometrySmoothing 1, gridSmoothing 1, attrTransferFilterType 1; flagColorSmoothing 0 (the CTC) leaves the sequence as it
 * is, a stream whose attribute-smoothing SEI sets it adds tmc2_codec_color_smoothing between the colour transfer and the
 * conversion to 8-bit RGB.
 * replaces: PCCCodec::identifyBoundaryPoints (PccLibCommon/source/PCCCodec.cpp:268-327), as generatePointCloud runs it
 * over all points when flagGeometrySmoothing is set (:955-976): PCCPointSet3::boundaryPointTypes_ becomes 0 / 1.     */
int tmc2_codec_identify_boundary_points( tmc2_frame* f );
/* replaces: PCCCodec::colorPointCloud (PCCCodec.cpp:1319-1460), branch "f < mapCount": every point takes the 16-bit colour
 * of its pixel in the decoded attribute frame of its map.  attribute: uint16 [2 maps][3 channels][H][W] (host memory),
 * i.e. context.getVideoAttributesMultiple()[0] frames 2f and 2f+1 after decoding + colour conversion.              */
int tmc2_codec_color_point_cloud( tmc2_frame* f, const uint16_t* attribute );
/* attribute == NULL above: the frames tmc2_codec_set_decoded_attribute_yuv420 left on the device are used.             */
/* replaces: PCCCodec::smoothPointCloudPostprocess (PCCCodec.cpp:54-148, gridSmoothing branch: addGridCentroid :982,
 * gridFiltering :1002, smoothPointCloudGrid :1067).  Boundary points that the trilinear blend of the cell centroids
 * pulls further than the threshold are moved there; their boundary type becomes 3.  Runs
 * tmc2_codec_identify_boundary_points first if that has not happened.  gridSize: an even size of 2 .. 64; any other is refused
 * (TMC2_E_UNSUPPORTED, the message names gridSize) before anything is allocated or launched, and the frame stays as it was --
 * with an odd size the 2x2x2 cells of a point next to the upper faces are not all inside the grid, and the reference writes
 * outside its cellIndex (PCCCodec.cpp:99-106).  A cell of more than 65535 points or a coordinate sum beyond 2^24 is refused too.  */
int tmc2_codec_smooth_point_cloud_postprocess( tmc2_frame* f, int gridSize, double thresholdSmoothing );
/* replaces: PCCPointSet3::transferColors16bitBP (PccLibCommon/source/PCCPointSet.cpp:1126-1470) with filterType 1 and the
 * arguments of PCCEncoder.cpp:657-672 / PCCDecoder.cpp:416-431: source = the cloud before smoothing with its 16-bit
 * colours, target = the smoothed cloud; only the moved points (boundary type 3) are recoloured.                     */
int tmc2_codec_transfer_colors_16bit_bp( tmc2_frame* f );
/* replaces: PCCCodec::colorSmoothing (PCCCodec.cpp:151-238: addGridColorCentroid :1170, gridFilteringColor :1193,
 * smoothPointCloudColorLC :1279) on the frame's finished cloud -- the branch "applyAttrSmoothingType_ != 0 &&
 * flagColorSmoothing_" of PCCEncoder.cpp:701-705 / PCCDecoder.cpp:463; call after tmc2_codec_transfer_colors_16bit_bp and before
 * tmc2_codec_convert_yuv16_to_rgb8.  gridSize = occupancyPrecision_ (what colorSmoothing reads; NOT the SEI's cgridSize_): 2, 4,
 * 8 or 16.  Boundary points (type 1) take the trilinear blend of the mean colours of the 2x2x2 grid cells around them when
 * its luma differs enough from their own; positions and boundary types do not change.  The patch of a point is taken as the
 * geometry smoothing takes it (blockToPatch through pointToPixel), the cube of the grid is 2^geometryBitDepth3D: the value
 * tmc2_segmenter_compute was given, or tmc2_frame_set_geometry_bit_depth_3d (a decoder-side frame has no other source).
 * TMC2_E_STATE without 16-bit colours or bit depth; TMC2_E_UNSUPPORTED for a cell of more than 65535 points (the reference's
 * uint16 count wraps) and for other grid sizes.                                                                        */
int tmc2_codec_color_smoothing( tmc2_frame* f, int gridSize, double thresholdColorSmoothing, double thresholdColorDifference,
                                double thresholdColorVariation );
int tmc2_frame_set_geometry_bit_depth_3d( tmc2_frame* f, int geometryBitDepth3D );
/* the same on host arrays (as tmc2_transfer_colors is to the frame entry): xyz int16[M][3], colors16 uint16[M][3] in / out,
 * boundaryType uint16[M], patchIndex uint32[M] (only equality of two points' values matters)                           */
int tmc2_color_smoothing( tmc2_ctx* ctx, const int16_t* xyz, uint16_t* colors16, const uint16_t* boundaryType, const uint32_t* patchIndex,
                          uint64_t M, int gridSize, int geometryBitDepth3D, double thresholdColorSmoothing,
                          double thresholdColorDifference, double thresholdColorVariation );
/* replaces: PCCPointSet3::convertYUV16ToRGB8 (PccLibCommon/include/PCCPointSet.h:133-166) */
int tmc2_codec_convert_yuv16_to_rgb8( tmc2_frame* f );
/* the finished cloud (any pointer may be NULL): positions int16[M][3] (smoothed once the smoothing ran), 16-bit colours
 * uint16[M][3], 8-bit colours uint8[M][3], boundary types uint16[M]; M = tmc2_frame_recon_count                     */
int tmc2_frame_get_post_reconstruction( tmc2_frame* f, int16_t* xyz, uint16_t* colors16, uint8_t* rgb, uint16_t* boundaryType );

/* ---- PCCMetrics ------------------------------------------------------------------------------------ */
/* replaces: PCCMetrics::compute for one frame (PccLibMetrics/source/PCCMetrics.cpp:324-375) with the defaults of
 * PCCMetricsParameters (dropDuplicates 2, neighborsProc 1, no Hausdorff): duplicate removal, normal copy / scaling,
 * QualityMetrics::compute both ways (:73-229) and their symmetric combination (:289-322).
 * srcNormals (double[n][3], the normals of the SOURCE cloud, e.g. from tmc2_frame_get_normals) may be NULL: no D2.
 * out[3][8]: rows A->B, B->A, symmetric; columns c2cMse, c2cPsnr, c2pMse, c2pPsnr, colorMse Y,U,V, colorPsnr Y.
 * counts[2]: points after duplicate removal (source, reconstruction).                                     */
int tmc2_metrics_compute( tmc2_ctx* ctx, const int16_t* srcXyz, const uint8_t* srcRgb, uint64_t n, const int16_t* recXyz,
                          const uint8_t* recRgb, uint64_t m, const double* srcNormals, double resolution, double* out,
                          int64_t* counts );

/* The same for a frame whose clouds are resident in HBM already (nothing is uploaded): source = the frame's points and colours
 * (and, with useNormals, its normals: tmc2_normals_compute / tmc2_frame_set_normals); reconstruction = which 0: what
 * tmc2_encoder_generate_attribute_images left (PCCCodec::generatePointCloud + transferColors), which 1: the finished cloud
 * of the post-reconstruction tail (tmc2_codec_smooth_point_cloud_postprocess .. tmc2_codec_convert_yuv16_to_rgb8: smoothed positions, final colours) -- what PccAppEncoder / PccAppDecoder hand to
 * PCCMetrics::compute (PccAppEncoder.cpp, metrics.compute( sources, reconstructs, normals ): PCCMetrics.cpp:324-375).        */
int tmc2_metrics_compute_frame( tmc2_frame* frame, int which, int useNormals, double resolution, double* out, int64_t* counts );
/* ... and for a frame that has no source cloud (the decoder side, tmc2_decoder_frame_create: PccAppDecoder reads the uncompressed
 * frames and their normals from PLY files and calls PCCMetrics::compute on them and the decoded clouds, PccAppDecoder.cpp): the
 * source comes from the host (as for tmc2_metrics_compute), the reconstruction is the frame's resident one (which: as above).   */
int tmc2_metrics_compute_frame_source( tmc2_frame* frame, int which, const int16_t* srcXyz, const uint8_t* srcRgb, uint64_t n,
                                       const double* srcNormals, double resolution, double* out, int64_t* counts );

/* The same three entries over the parameter space of PCCMetricsParameters that PccAppMetrics takes on its command line
 * (reflectance and lidar excepted: these clouds carry neither).  tmc2_metrics_params_default: computeC2c 1, computeC2p 1,
 * computeColor 1, computeHausdorff 0, dropDuplicates 2, neighborsProc 1 -- with these the _ex entries run what the entries
 * above run and return their bits in columns 0-7.
 * out[3][14]: columns 0-7 as above; 8, 9 colorPsnr U, V; 10 c2cHausdorff, 11 c2cHausdorffPsnr, 12 c2pHausdorff, 13
 * c2pHausdorffPsnr.  What a flag turns off stays 0, as QualityMetrics' constructor leaves it.
 * dropDuplicates 0: no de-duplication and no reordering (counts = 0, 0; duplicated source points all take the normal of the LAST
 * duplicate, PCCPointSet3::copyNormals); 1: a run of equal positions keeps the colour of its first point; 2: the mean colour.
 * neighborsProc 0: the colour of the first search result; 1, 2: the rounded mean over the points at the minimum distance; 3, 4 AS
 * THE REFERENCE IS WRITTEN (PCCMetrics.cpp:155-171: distBest and indexBest start at 0, strict comparisons, indexBest names a point
 * of the other cloud): 3 takes the colour of that cloud's point 0, 4 the first member of the group, in ascending index, whose
 * colour distance strictly beats every earlier one -- point 0 again if all are 0.
 * computeHausdorff: the maxima start at DBL_MIN (two identical clouds report it).  computeC2p is ignored without normals.
 * TMC2_E_INVALID for params == NULL; TMC2_E_UNSUPPORTED (nothing is launched) for a flag that is not 0 / 1, dropDuplicates
 * outside 0..2, neighborsProc outside 0..4.                                                                          */
typedef struct tmc2_metrics_params {
  int32_t computeC2c, computeC2p, computeColor, computeHausdorff;
  int32_t dropDuplicates;
  int32_t neighborsProc;
} tmc2_metrics_params;
void tmc2_metrics_params_default( tmc2_metrics_params* params );
int tmc2_metrics_compute_ex( tmc2_ctx* ctx, const int16_t* srcXyz, const uint8_t* srcRgb, uint64_t n, const int16_t* recXyz,
                             const uint8_t* recRgb, uint64_t m, const double* srcNormals, double resolution,
                             const tmc2_metrics_params* params, double* out, int64_t* counts );
int tmc2_metrics_compute_frame_ex( tmc2_frame* frame, int which, int useNormals, double resolution, const tmc2_metrics_params* params,
                                   double* out, int64_t* counts );
int tmc2_metrics_compute_frame_source_ex( tmc2_frame* frame, int which, const int16_t* srcXyz, const uint8_t* srcRgb, uint64_t n,
                                          const double* srcNormals, double resolution, const tmc2_metrics_params* params, double* out,
                                          int64_t* counts );

/* The accumulation of QualityMetrics::compute alone (`sseC2c += ..`, `sseC2p += ..`, `sseColor[i] += ..` over the points in
 * index order, PCCMetrics.cpp:187-198) for per-point terms the caller holds on the host: termsA[nA][5] / termsB[nB][5] = the
 * squared distance (an integer), the point-to-plane term and the three colour terms of every point, one direction each (either
 * may be empty).  out[10]: the five sums of A, then of B -- the doubles the reference's loop leaves, bit for bit (the ordered
 * fp64 sums are evaluated block-wise in exact integer arithmetic: csrc/ordered_sum.h).  What tmc2_metrics_compute* run
 * internally on the device-resident terms; exported so that the form can be checked on arbitrary terms.                */
int tmc2_metrics_ordered_sums( tmc2_ctx* ctx, const double* termsA, uint64_t nA, const double* termsB, uint64_t nB, double* out );

/* replaces: PCCMetrics::display / QualityMetrics::print (PCCMetrics.cpp:376-391, 230-279) for one frame: the text the CTC log
 * parsers read, from the numbers of tmc2_metrics_compute (out[3][8], counts[2]), the point counts before duplicate removal
 * and the peak value.  precision: that of the application's std::cout (PccAppEncoder / PccAppMetrics set 9).  text may be
 * NULL to query the size (*needed, including the terminating 0).  Host only.                                       */
int tmc2_metrics_display( const double* out, uint64_t sourcePoints, uint64_t reconstructPoints, const int64_t* counts,
                          uint64_t resolution, int withC2p, int precision, char* text, uint64_t capacity, uint64_t* needed );
/* ... from out[3][14] of the _ex entries and their parameters: rows 1 and 2 print the blocks the flags leave on, the Hausdorff
 * lines among them (the "p2plane" ones print the p2point members, as QualityMetrics::print does); the symmetric row prints as
 * the reference's does -- it is a QualityMetrics with DEFAULT parameters (operator+ sets none): all of point-to-point,
 * point-to-plane and colour, no Hausdorff lines.  All three colour PSNR lines come from columns 7-9.  withC2p: normals were given. */
int tmc2_metrics_display_ex( const double* out, const tmc2_metrics_params* params, uint64_t sourcePoints, uint64_t reconstructPoints,
                             const int64_t* counts, uint64_t resolution, int withC2p, int precision, char* text, uint64_t capacity,
                             uint64_t* needed );

/* ---- point-cloud ingest and conformance checksums (host; no device needed) ------------------------------------------- */
/* replaces: PCCPointSet3::read (PccLibCommon/source/PCCPointSet.cpp:464-757) as PCCGroupOfFrames::load (PCCGroupOfFrames.cpp:
 * 46-80) calls it per frame: ASCII and binary_little_endian PLY, x / y / z of 2, 4 or 8 bytes, uchar red / green / blue, float
 * nx / ny / nz (binary bodies only, as in the reference); other vertex properties are skipped.  The cloud lands directly in
 * the caller's buffers -- xyz int16[capacity][3], rgb uint8[capacity][3] (may be NULL), normals double[capacity][3] (NULL:
 * not read) -- e.g. the page-locked staging the upload reads.  threads: parser threads (0 = 8).
 * tmc2_ply_info only reads the header (pointCount, whether red/green/blue resp. float normals are present).          */
int tmc2_ply_info( const char* path, int readNormals, uint64_t* pointCount, int* hasColors, int* hasNormals );
int tmc2_ply_read( const char* path, int16_t* xyz, uint8_t* rgb, double* normals, uint64_t capacity, int threads,
                   uint64_t* pointCount );
/* replaces: PCCPointSet3::write (PCCPointSet.cpp:359-462): the PLY file the reference writes for a reconstructed or decoded
 * frame, byte for byte (ASCII or binary_little_endian; rgb / normals may be NULL)                                  */
int tmc2_ply_write( const char* path, const int16_t* xyz, const uint8_t* rgb, const double* normals, uint64_t n, int asAscii );
/* replaces: PCCPointSet3::computeChecksum( reorderPoints ) / computeMd5 / reorder (PCCPointSet.cpp:222-305): the MD5 the
 * conformance logs carry, over int16 positions then uint8 colours (rgb may be NULL); reorderPoints sorts by (x, y, z) and
 * merges points that share a position (mean colour) first.                                                        */
int tmc2_point_set_checksum( const int16_t* xyz, const uint8_t* rgb, uint64_t n, int reorderPoints, uint8_t digest[16] );

/* replaces: PCCChecksum::write / read (PccLibMetrics/source/PCCChecksum.cpp:112-139): the ".checksum" file kept next to the
 * bitstream, one line per frame.  digests: uint8[frames][16] (tmc2_point_set_checksum).  read: digests may be NULL to query
 * the frame count.                                                                                                  */
int tmc2_checksum_file_write( const char* path, const uint8_t* digests, uint64_t frames );
int tmc2_checksum_file_read( const char* path, uint8_t* digests, uint64_t capacity, uint64_t* frames );

/* ---- host-only pieces of the path (no device needed; used by the CPU test tier) -------------- */
/* the nanoflann-identical tree builder behind tmc2_frame_create: perm = tree order -> original index */
int tmc2_host_kdtree_build( const int16_t* xyz, uint64_t n, uint32_t* perm, uint64_t* nodeCount, int32_t* depth );
/* the placement logic behind tmc2_encoder_pack_flexible on plain records: patches by index (u0 / v0 / patchOrientation out),
 * their block-occupancy pool; order = list order out */
int tmc2_host_pack_flexible( tmc2_patch* patches, int count, const uint8_t* occupancy, int presetWidth, int numTilesHor,
                             double tileHeightToWidthRatio, int32_t* order, int32_t* height );
/* the placement logic behind tmc2_encoder_pack_spatial_consistency on plain records: patches by index (u0 / v0 /
 * patchOrientation out), their block-occupancy pool, the previous frame's patches in list order */
/* the allocation behind tmc2_encoder_global_patch_allocation on plain records.  counts[frames]; patches / matches: all
 * frames back to back, each IN LIST ORDER (in / out); occupancy + occupancyBase[f]: frame f's block-occupancy pool
 * (patch.occOffset is relative to it); tileWidth / tileHeight: the common tile size after resizeTileGeometryVideo.
 * Out: the rebuilt pools back to back in occupancyOut (frame f at occupancyOutBase[f]; occupancyOutBase[frames] = bytes
 * needed -- TMC2_E_INVALID if that exceeds occupancyOutCapacity), the tile size of every frame.                      */
int tmc2_host_global_patch_allocation( int frames, int32_t* counts, tmc2_patch* patches, const uint8_t* occupancy,
                                       const int64_t* occupancyBase, int32_t* matches, int tileWidth, int tileHeight,
                                       int minimumImageWidth, int minimumImageHeight, uint8_t* occupancyOut,
                                       int64_t occupancyOutCapacity, int64_t* occupancyOutBase, int32_t* widths,
                                       int32_t* heights );
int tmc2_host_pack_spatial_consistency( tmc2_patch* patches, int count, const uint8_t* occupancy, const tmc2_patch* previous,
                                        int previousCount, int presetWidth, int numTilesHor, double tileHeightToWidthRatio,
                                        int32_t* order, int32_t* matches, int32_t* height );
/* replaces: PCCEncoder::placeSegments (PccLibEncoder/source/PCCEncoder.cpp:4790-4840) over the patch RECORDS of a whole GOF
 * -- what the rank that holds the records of all frames runs when the frames themselves live on several GPUs.
 * mode 0: packFlexible per frame; 1: frame f > 0 packed against frame f-1 (spatialConsistencyPackFlexible); 2: that chain
 * followed by performDataAdaptiveGPAMethod.  counts[frames]; patches: all frames back to back, in: by index (occOffset
 * into occupancy + occupancyBase[f]), out: in LIST order with placements (occOffset into occupancyOut +
 * occupancyOutBase[f]); matches: out, per list position; widths / heights: the tile each frame is left with (may be NULL).
 * The number of records per frame does not change.  occupancyOutBase has frames + 1 entries (the last = bytes used).    */
int tmc2_host_place_segments( int frames, const int32_t* counts, tmc2_patch* patches, const uint8_t* occupancy,
                              const int64_t* occupancyBase, int mode, int minimumImageWidth, int minimumImageHeight, int numTilesHor,
                              double tileHeightToWidthRatio, int32_t* matches, uint8_t* occupancyOut, int64_t occupancyOutCapacity,
                              int64_t* occupancyOutBase, int32_t* widths, int32_t* heights );
/* the exact spanning-tree orientation behind tmc2_normals_orient (normals in/out, knn = [n][k]) */
int tmc2_host_orient_normals( const int16_t* xyz, uint64_t n, const uint32_t* knn, int k, double* normals );
/* the exact restatement of PCCCodec::colorSmoothing behind tmc2_color_smoothing / tmc2_codec_color_smoothing (same arrays) */
int tmc2_host_color_smoothing( const int16_t* xyz, uint16_t* colors16, const uint16_t* boundaryType, const uint32_t* patchIndex,
                               uint64_t M, int gridSize, int geometryBitDepth3D, double thresholdColorSmoothing,
                               double thresholdColorDifference, double thresholdColorVariation );
/* PCCMetrics::compute for one frame restated on the host (csrc/metrics_host.cpp; no device, brute-force neighbour search): the
 * arguments and results of tmc2_metrics_compute_ex.  It does not know the k-d tree's visiting order; where the answer depends on
 * it -- the first result among several equidistant points (neighborsProc 0), a minimum-distance group of more than 30 points, the
 * floating-point sum over the nearest source points of a reconstructed point nobody voted for, unless every order of adding
 * them gives the same doubles -- it returns
 * TMC2_E_ORDER and leaves out untouched.                                                                              */
int tmc2_host_metrics_compute( const int16_t* srcXyz, const uint8_t* srcRgb, uint64_t n, const int16_t* recXyz, const uint8_t* recRgb,
                               uint64_t m, const double* srcNormals, double resolution, const tmc2_metrics_params* params, double* out,
                               int64_t* counts );
/* the exact restatement of PatchBlockFiltering::patchBorderFiltering (PCCPatch.cpp:950-976) behind
 * tmc2_codec_generate_point_cloud_pbf, on host arrays: patch records in list order, the occupancy video (uint8 [H/p][W/p]),
 * geometry map 0 (uint16 [H][W]), blockToPatch (uint32 [H/16][W/16], list position + 1); occupancy / border as
 * tmc2_frame_get_patch_border_filtering returns them (either may be NULL)                                               */
int tmc2_host_patch_border_filtering( const tmc2_patch* patches, int count, int width, int height, int occupancyPrecision,
                                      const uint8_t* occVideo, const uint16_t* geometryD0, const uint32_t* blockToPatch,
                                      int thresholdLossyOM, int passesCount, int filterSize, int log2Threshold, uint8_t* occupancy,
                                      uint8_t* border );
/* the same rule compiled for the host (csrc/voxelize.h; no device): what tmc2_segmenter_convert_points_to_voxels is checked against */
int tmc2_host_convert_points_to_voxels( const int16_t* xyz, uint64_t n, int voxDim, int bits, int16_t* voxelXyz, uint64_t* voxelCount,
                                        uint32_t* voxelOfPoint );
/* PCCPatchSegmenter3::refineSegmentation restated on the host (csrc/refine_knn_host.cpp; no device) over tmc2_host_kdtree_build's
 * tree: normals double[n][3], partition uint32[n] in and out (labels 0..5); adjacency uint32[n][maxNNCount] takes the rows of
 * nanoflann's search in its result order, or NULL.  Refusals as tmc2_segmenter_refine.                                    */
int tmc2_host_refine_segmentation( const int16_t* xyz, uint64_t n, const double* normals, uint32_t* partition, int maxNNCount,
                                   double lambda, int iterationCount, uint32_t* adjacency /* [n][maxNNCount], may be NULL */ );
/* PCCPointSet3::transferColors restated on the host (csrc/color_transfer_host.cpp; no device): nanoflann's searches over
 * tmc2_host_kdtree_build's trees, libstdc++'s std::sort of the backward lists replayed, and the per-target rules of
 * csrc/color_transfer_rules.h -- the text the device kernels run.  Arguments and refusals as tmc2_transfer_colors_ex.        */
int tmc2_host_transfer_colors( const int16_t* srcXyz, const uint8_t* srcRgb, uint64_t n, const int16_t* tgtXyz, uint64_t m,
                               const tmc2_color_transfer_params* params, uint8_t* tgtRgb );

/* ---- the shared device primitives on their own (csrc/selftest.hip; DESIGN.md "primitives under test") ------------------- */
/* What the stages are built on, reachable without a stage so that it can be compared with a plain loop at shapes no cloud produces.
 * Every d_ pointer is DEVICE memory of the context's device (tmc2_ctx_device_alloc / tmc2_ctx_upload / tmc2_ctx_download); the
 * calls are queued on the context's stream and NOT waited for.  They read the context's options as the stages do.  Not part of the
 * drop-in boundary: the reference has no counterpart.
 * scan: exclusiveScanU32 as the stages call it -- d_out may be d_in; d_total may be NULL; hostAnswer (page-locked: tmc2_host_alloc)
 * may be NULL, else it receives the total and, behind it, carryWords <= 7 words of d_carry.  epoch != 0 first sets the context's
 * scan epoch (30 bits): the wrap is 2^30 scans away otherwise.                                                          */
int tmc2_selftest_scan( tmc2_ctx* ctx, const uint32_t* d_in, uint32_t* d_out, uint64_t n, uint32_t* d_total, uint32_t* hostAnswer,
                        const uint32_t* d_carry, int carryWords, uint64_t epoch );
/* fill: fillRegions over regions[count][3] = (device address, bytes, byte value), a HOST array; count <= 13, of which fillRegions
 * itself refuses the thirteenth region that is not empty.                                                                  */
int tmc2_selftest_fill( tmc2_ctx* ctx, const uint64_t* regions, int count );
/* work map: one lane per element on the helpers of the XCD work mapping.  d_hits[2][n] += 1 at the lane's chunkedIndex() resp.
 * pointOfLane() element; d_logical[gridBlocks] = the logical block of each workgroup.  gridBlocks 0: chunkedGrid of the blocks n
 * needs, as the stages size a pass.  liveBlocks != 0: the form of the k-NN kernel (a grid of a multiple of 8 blocks, the eighths
 * are those of the live blocks, a surplus workgroup leaves and records 0xFFFFFFFF; d_hits[1] = d_hits[0]).               */
int tmc2_selftest_work_map( tmc2_ctx* ctx, uint64_t gridBlocks, int blockThreads, uint64_t n, uint64_t liveBlocks, uint32_t* d_hits,
                            uint32_t* d_logical );
/* components: S7's own kernels (mutual mask, initial forest, union pass, the UF_CHECK pass if the option is set, the find of the
 * flatten pass) on a neighbour table d_knn[n][16] (a row is padded with the point itself), planes d_partition[n], d_raw[n] (0: the
 * point takes no part), d_perm[n] (the order MUTUAL_ORDER=tree walks; may be NULL).  d_root[u]: the root of every raw point;
 * d_bad[2]: broken links / split edges as UF_CHECK counts them (the caller clears it).                                    */
int tmc2_selftest_components( tmc2_ctx* ctx, const uint32_t* d_knn, const uint8_t* d_partition, const uint8_t* d_raw,
                              const uint32_t* d_perm, uint64_t n, uint32_t* d_root, uint32_t* d_bad );
/* union-find over an edge list: d_word[n] in: a forest whose links fall in priority (parity 0: the parent; else parent << 1 |
 * parity), out: the settled words; d_edges[m][3] = (a, b, s: the parity of a relative to b).  One launch runs the store-free
 * pre-check (if precheck) and the union of every edge, a second the find of every element into d_root / d_rootParity, a third the
 * coherent climb: d_bad[0] += links that do not fall in priority or leave [0, n) and edges with an end outside it, d_bad[1] +=
 * edges whose ends have two roots (the caller clears both).  agent: every load at agent scope.                             */
int tmc2_selftest_union_find( tmc2_ctx* ctx, int parity, uint32_t* d_word, uint64_t n, const uint32_t* d_edges, uint64_t m, int precheck,
                              int agent, uint32_t* d_root, uint32_t* d_rootParity, uint32_t* d_bad );
/* CandSort::sort, one list per lane: d_lists[total][2] = (distance, payload), list l = [d_offsets[l], d_offsets[l + 1]); d_ok[l] =
 * 0 where the depth limit was reached.  std_sort: the real std::sort( .., dist < dist ) over the same layout in HOST memory.     */
int tmc2_selftest_cand_sort( tmc2_ctx* ctx, uint32_t* d_lists, const uint32_t* d_offsets, uint64_t lists, uint32_t* d_ok );
int tmc2_selftest_std_sort( uint32_t* lists, const uint32_t* offsets, uint64_t count );
/* marked cells: markedCells (csrc/cell_grid.hip) as T3 and T6 call it, over d_xyz4[M][4] (x, y, z, 0) and d_boundaryType[M] (bytes), on
 * the grid of gridSize (even, 2 .. 64) over the cube of 2^bits (bits != 0, T6's) or over [0, maxCoord] (bits == 0, T3's); at most 2^31
 * cells.  The eight cells around every type-1 point inside the faces are marked.  *cells (HOST): their number -- this entry waits
 * for it.  d_bits / d_rank [ceil( w^3 / 32 )] (each may be NULL): one bit per cell in raster order, and per word the marked cells
 * before it.  d_slots[keys]: slotOfKey of every cell key of d_keys -- its rank among the marked cells, 0xFFFFFFFF if not marked.  */
int tmc2_selftest_marked_cells( tmc2_ctx* ctx, const int16_t* d_xyz4, const uint8_t* d_boundaryType, uint64_t M, int gridSize, int bits,
                                int maxCoord, uint32_t* cells, uint32_t* d_bits, uint32_t* d_rank, const uint32_t* d_keys, uint64_t keys,
                                uint32_t* d_slots );
/* wave: the cross-lane idioms of csrc/wave.h, one per call, over n elements (at most 2^24, a whole number of groups).
 * op 0 .. 5: waveInclusive, waveInclusive<16>, waveSum, waveSum<16>, waveMin, waveMax on d_in[n] -> d_out[n], one value per lane,
 *   workgroups of 256; param = the element type (0: uint32, 1: int32, 2: double).
 * op 6: laneRank through a compaction, workgroups of 256: every wavefront writes the numbers of its lanes with d_in[i] != 0 back to
 *   back into its 64 words of d_out (the rest: 0xFFFFFFFF); d_aux[i] = the wavefront's count.
 * op 7: ldsBitonicSort of lists of param keys (a power of two, 64 .. 8192), one wavefront each: d_in[n] -> d_out[n].
 * op 8: blockExclusive over workgroups of param (1, 2, 4, 16) wavefronts: d_out[i] = the sum of the workgroup's values before
 *   thread i, d_aux[i] = the workgroup's total.  (uint32 for op 6 .. 8; d_aux may be NULL for op 0 .. 5 and 7.)               */
int tmc2_selftest_wave( tmc2_ctx* ctx, int op, int param, const void* d_in, void* d_out, uint32_t* d_aux, uint64_t n );
/* pool probe: a buffer of `bytes` (1 .. 2^30) from the context's pool, as every stage gets its temporaries, downloaded over its whole
 * size class to hostOut (HOST memory of *classBytes bytes: the next power of two, at least 256; hostOut NULL: only *classBytes is
 * reported) and released -- on purpose a reader of memory it has not written.  Under option POOL_POISON every byte is the poison
 * byte; without it the content is unspecified.  This entry waits.  pool poisoned: the blocks the pool has filled so far.          */
int tmc2_selftest_pool_probe( tmc2_ctx* ctx, uint64_t bytes, uint8_t* hostOut, uint64_t* classBytes );
int tmc2_selftest_pool_poisoned( tmc2_ctx* ctx, uint64_t* blocks );

#ifdef __cplusplus
}
#endif
#endif /* TMC2HIP_H */
