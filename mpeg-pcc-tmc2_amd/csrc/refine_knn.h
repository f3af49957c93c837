// refine_knn.h -- the k-NN refinement of the segmentation (the reference's non-grid mode), the rules host and device share.
//
// Replaces the arithmetic of PCCPatchSegmenter3::refineSegmentation (PccLibEncoder/source/PCCPatchSegmenter.cpp:1322-1384):
//   weight = lambda / maxNNCount; per round and point: count[j] = neighbours whose CURRENT plane is j, the plane stays partition[i]
//   unless some score = normal . orientation[j] + weight * count[j] is strictly above the best so far, which starts at 0.0.
// The six orientations are the signed unit axes +x +y +z -x -y -z; the dot product is formed in full, left to right, as
// PCCVector3D::operator* does (a NaN or an infinity in a normal travels as it does there).  No FMA: -ffp-contract=off.
//
// The neighbourhood of a point is the SET nanoflann's search returns for maxNNCount results: the first K points under the key
// (squared distance, position in the query's own depth-first visiting order) -- near child first at every split, tree order inside
// a leaf, a candidate inserted behind every entry of equal distance and dropped when it equals the worst of a full list.
#pragma once
#include <cstdint>

#if defined( __HIPCC__ )
#define TMC2_REFINE_FN __host__ __device__ __forceinline__
#else
#define TMC2_REFINE_FN inline
#endif

namespace tmc2 {

constexpr int kWideMaxK = 1024;  // the wave-per-query search keeps its list in LDS: 8 bytes per entry and wave

// the plane of a point after one round
TMC2_REFINE_FN uint32_t refineVote( double nx, double ny, double nz, uint32_t current, const uint32_t count[6], double weight ) {
  uint32_t best      = current;
  double   bestScore = 0.0;
  for ( uint32_t j = 0; j < 6; ++j ) {
    const double s           = j < 3 ? 1.0 : -1.0;
    const double ox          = j % 3 == 0 ? s : 0.0, oy = j % 3 == 1 ? s : 0.0, oz = j % 3 == 2 ? s : 0.0;
    const double scoreNormal = nx * ox + ny * oy + nz * oz;
    const double score       = scoreNormal + weight * double( count[j] );
    if ( score > bestScore ) {
      bestScore = score;
      best      = j;
    }
  }
  return best;
}

// What tmc2_segmenter_refine and tmc2_host_refine_segmentation refuse: nullptr, or a printf format (at most one int: the offending value)
inline const char* refineKnnRefusal( int maxNNCount, double lambda, int iterationCount, int* offending ) {
  if ( maxNNCount < 1 || maxNNCount > kWideMaxK ) {
    *offending = maxNNCount;
    return "maxNNCountRefineSegmentation %d outside 1..1024 (the search keeps its result list in LDS)";
  }
  if ( iterationCount < 0 ) {
    *offending = iterationCount;
    return "iterationCountRefineSegmentation %d is negative";
  }
  if ( !( lambda >= 0.0 ) ) {
    *offending = 0;
    return "lambdaRefineSegmentation is negative or not a number";
  }
  return nullptr;
}

}  // namespace tmc2
