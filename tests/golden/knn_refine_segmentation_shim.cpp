// knn_refine_segmentation_shim.cpp -- FIXTURE GENERATION ONLY (tests/golden/make_knn_refine_segmentation_golden.py compiles it into
// a temporary directory against oracle/_ref/libtmc2ref.so and the reference's headers; never part of the product library, never
// built by build()).  Entries on plain arrays, all through public members of the unmodified reference:
//   krs_adjacency   PCCPatchSegmenter3::computeAdjacencyInfo: the rows of PCCKdTree::search( query, K ) for the cloud's own points or
//                   for foreign queries against the cloud's tree
//   krs_rounds      PCCNormalsGenerator3::compute, initialSegmentation (the initial partition), then refineSegmentation from that
//                   partition once per listed round count
//   krs_compute     PCCPatchSegmenter3::compute with gridBasedRefineSegmentation_ as the parameters say, gridBasedSegmentation_ set or
//                   not; krs_patches: the patch list it appended (22 record fields, both depth maps, block occupancy)
// ip: the 20 int32 fields of the parameter struct in its order (tests/oracle_binding.SegParams), dp: its 6 doubles.
#include "PCCCommon.h"
#include "PCCPointSet.h"
#include "PCCKdTree.h"
#include "PCCNormalsGenerator.h"
#include "PCCPatch.h"
#include "PCCPatchSegmenter.h"

#include <chrono>
#include <iostream>
#include <limits>
#include <sstream>

namespace {
using namespace pcc;

struct Hush {  // the segmenter reports its progress on std::cout
  std::streambuf*    saved;
  std::ostringstream sink;
  Hush() : saved( std::cout.rdbuf( sink.rdbuf() ) ) {}
  ~Hush() { std::cout.rdbuf( saved ); }
};

void cloudOf( PCCPointSet3& cloud, const int16_t* xyz, const uint8_t* rgb, size_t n ) {
  cloud.resize( n );
  cloud.addColors();
  for ( size_t i = 0; i < n; ++i ) {
    cloud[i] = PCCPoint3D( xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2] );
    cloud.setColor( i, PCCColor3B( rgb[3 * i], rgb[3 * i + 1], rgb[3 * i + 2] ) );
  }
}

void paramsOf( PCCPatchSegmenter3Parameters& q, const int32_t* ip, const double* dp, int gridBased, int voxDim ) {
  q.gridBasedSegmentation_               = gridBased != 0;
  q.voxelDimensionGridBasedSegmentation_ = size_t( voxDim );
  q.nnNormalEstimation_                  = size_t( ip[0] );
  q.normalOrientation_                   = size_t( ip[1] );
  q.gridBasedRefineSegmentation_         = ip[2] != 0;
  q.maxNNCountRefineSegmentation_        = size_t( ip[3] );
  q.iterationCountRefineSegmentation_    = size_t( ip[4] );
  q.voxelDimensionRefineSegmentation_    = size_t( ip[5] );
  q.searchRadiusRefineSegmentation_      = size_t( ip[6] );
  q.occupancyResolution_                 = size_t( ip[7] );
  q.enablePatchSplitting_                = ip[8] != 0;
  q.maxPatchSize_                        = size_t( ip[9] );
  q.quantizerSizeX_                      = size_t( ip[10] );
  q.quantizerSizeY_                      = size_t( ip[11] );
  q.minPointCountPerCCPatchSegmentation_ = size_t( ip[12] );
  q.maxNNCountPatchSegmentation_         = size_t( ip[13] );
  q.surfaceThickness_                    = size_t( ip[14] );
  q.mapCountMinus1_                      = size_t( ip[15] );
  q.minLevel_                            = size_t( ip[16] );
  q.maxAllowedDepth_                     = size_t( ip[17] );
  q.geometryBitDepth2D_                  = size_t( ip[18] );
  q.geometryBitDepth3D_                  = size_t( ip[19] );
  q.maxAllowedDist2RawPointsDetection_   = dp[0];
  q.maxAllowedDist2RawPointsSelection_   = dp[1];
  q.lambdaRefineSegmentation_            = dp[2];
  q.weightNormal_                        = PCCVector3D( dp[3], dp[4], dp[5] );
  q.EOMFixBitCount_                      = 2;
  q.EOMSingleLayerMode_                  = false;
  q.useEnhancedOccupancyMapCode_         = false;
  q.absoluteD1_                          = true;
  q.createSubPointCloud_                 = false;
  q.surfaceSeparation_                   = false;
  q.additionalProjectionPlaneMode_       = 0;
  q.partialAdditionalProjectionPlane_    = 0.0;
  q.patchExpansion_                      = false;
  q.highGradientSeparation_              = false;
  q.minGradient_                         = 15.0;
  q.minNumHighGradientPoints_            = 256;
  q.enablePointCloudPartitioning_        = false;
  q.numTilesHor_                         = 2;
  q.tileHeightToWidthRatio_              = 1.0;
  q.numCutsAlong1stLongestAxis_          = 1;
  q.numCutsAlong2ndLongestAxis_          = 1;
  q.numCutsAlong3rdLongestAxis_          = 1;
}

std::vector<PCCPatch> g_list;  // what the last krs_compute appended

void geometryOf( PCCPointSet3& cloud, const int16_t* xyz, size_t n ) {
  cloud.resize( n );
  for ( size_t i = 0; i < n; ++i ) cloud[i] = PCCPoint3D( xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2] );
}
}  // namespace

// rows uint32 [nq][K]; queries null: the cloud's own points.  A row shorter than K (never, for K <= n) is padded with 0xFFFFFFFF.
extern "C" void krs_adjacency( const int16_t* xyz, size_t n, const int16_t* queries, size_t nq, int K, uint32_t* rows ) {
  Hush         hush;
  PCCPointSet3 cloud, asked;
  geometryOf( cloud, xyz, n );
  if ( queries ) geometryOf( asked, queries, nq );
  PCCKdTree          tree( cloud );
  PCCPatchSegmenter3 segmenter;
  segmenter.setNbThread( 1 );
  std::vector<std::vector<size_t>> adj;
  segmenter.computeAdjacencyInfo( queries ? asked : cloud, tree, adj, size_t( K ) );
  for ( size_t i = 0; i < adj.size(); ++i )
    for ( size_t j = 0; j < size_t( K ); ++j ) rows[i * size_t( K ) + j] = j < adj[i].size() ? uint32_t( adj[i][j] ) : 0xFFFFFFFFu;
}

// initial uint32 [n]; partitions uint8 [counts][n]: the partition after roundCounts[c] rounds, each from the initial one
extern "C" void krs_rounds( const int16_t* xyz, const uint8_t* rgb, size_t n, const int32_t* ip, const double* dp, const int32_t* roundCounts,
                            int counts, uint32_t* initial, uint8_t* partitions, double* seconds ) {
  Hush         hush;
  PCCPointSet3 cloud;
  cloudOf( cloud, xyz, rgb, n );
  PCCPatchSegmenter3Parameters q;
  paramsOf( q, ip, dp, 0, 0 );
  PCCPatchSegmenter3 segmenter;
  segmenter.setNbThread( 1 );
  PCCKdTree            tree( cloud );
  PCCNormalsGenerator3 generator;
  const double         mx = ( std::numeric_limits<double>::max )();
  const PCCNormalsGenerator3Parameters g = {PCCVector3D( 0.0 ), mx, mx, mx, mx, q.nnNormalEstimation_, q.nnNormalEstimation_, q.nnNormalEstimation_, 0,
                                            static_cast<PCCNormalsGeneratorOrientation>( q.normalOrientation_ ), false, false, false};
  generator.compute( cloud, tree, g, 1 );
  // (the six projection planes -- +x +y +z -x -y -z, additionalProjectionPlaneMode_ 0 -- are private members of the segmenter)
  PCCVector3D planes[6];
  for ( int k = 0; k < 6; ++k ) planes[k] = PCCVector3D( 0.0 ), planes[k][k % 3] = k < 3 ? 1.0 : -1.0;
  std::vector<size_t> first;
  segmenter.initialSegmentation( cloud, generator, planes, 6, first, q.weightNormal_ );
  for ( size_t i = 0; i < n; ++i ) initial[i] = uint32_t( first[i] );
  for ( int c = 0; c < counts; ++c ) {
    std::vector<size_t> labels = first;
    const auto          t0     = std::chrono::steady_clock::now();
    segmenter.refineSegmentation( cloud, tree, generator, planes, 6, q.maxNNCountRefineSegmentation_, q.lambdaRefineSegmentation_,
                                  size_t( roundCounts[c] ), labels );
    seconds[c] = std::chrono::duration<double>( std::chrono::steady_clock::now() - t0 ).count();
    for ( size_t i = 0; i < n; ++i ) partitions[size_t( c ) * n + i] = uint8_t( labels[i] );
  }
}

// -> number of patches; sizes[0] / sizes[1]: entries of the depth pools / of the occupancy pool; *seconds: compute() alone
extern "C" int krs_compute( const int16_t* xyz, const uint8_t* rgb, size_t n, const int32_t* ip, const double* dp, int gridBased, int voxDim,
                            int64_t* sizes, double* seconds ) {
  Hush         hush;
  PCCPointSet3 cloud;
  cloudOf( cloud, xyz, rgb, n );
  PCCPatchSegmenter3Parameters q;
  paramsOf( q, ip, dp, gridBased, voxDim );
  PCCPatchSegmenter3 segmenter;
  segmenter.setNbThread( 1 );
  g_list.clear();
  g_list.reserve( 256 );
  std::vector<PCCPointSet3> subClouds;
  float                     distanceSrcRec = 0;
  const auto                t0             = std::chrono::steady_clock::now();
  segmenter.compute( cloud, 0, q, g_list, subClouds, distanceSrcRec );
  if ( seconds ) *seconds = std::chrono::duration<double>( std::chrono::steady_clock::now() - t0 ).count();
  sizes[0] = sizes[1] = 0;
  for ( auto& p : g_list ) sizes[0] += int64_t( p.getSizeU() * p.getSizeV() ), sizes[1] += int64_t( p.getSizeU0() * p.getSizeV0() );
  return int( g_list.size() );
}

// records int32 [count][22] in the order of tests/param_cases.PATCH_FIELDS; depth0 / depth1 int16, occupancy uint8: the pools
extern "C" void krs_patches( int32_t* records, int16_t* depth0, int16_t* depth1, uint8_t* occupancy ) {
  size_t d = 0, o = 0;
  for ( size_t k = 0; k < g_list.size(); ++k ) {
    auto&         p    = g_list[k];
    const int32_t f[22] = {int32_t( p.getIndex() ),       int32_t( p.getViewId() ),        int32_t( p.getNormalAxis() ),
                           int32_t( p.getTangentAxis() ), int32_t( p.getBitangentAxis() ), int32_t( p.getProjectionMode() ),
                           int32_t( p.getU1() ),          int32_t( p.getV1() ),            int32_t( p.getD1() ),
                           int32_t( p.getSizeU() ),       int32_t( p.getSizeV() ),         int32_t( p.getSizeD() ),
                           int32_t( p.getSizeDPixel() ),  int32_t( p.getSizeU0() ),        int32_t( p.getSizeV0() ),
                           int32_t( p.getPatchSize2DXInPixel() ), int32_t( p.getPatchSize2DYInPixel() ), int32_t( p.getD0Count() ),
                           int32_t( p.getEOMandD1Count() ), int32_t( p.getU0() ),          int32_t( p.getV0() ),
                           int32_t( p.getPatchOrientation() )};
    for ( int j = 0; j < 22; ++j ) records[22 * k + j] = f[j];
    const size_t pixels = p.getSizeU() * p.getSizeV(), blocks = p.getSizeU0() * p.getSizeV0();
    const auto & a = p.getDepth( 0 ), &b = p.getDepth( 1 );
    for ( size_t j = 0; j < pixels; ++j ) depth0[d + j] = a[j], depth1[d + j] = b.size() == pixels ? b[j] : a[j];
    for ( size_t j = 0; j < blocks; ++j ) occupancy[o + j] = p.getOccupancy()[j] ? 1 : 0;
    d += pixels, o += blocks;
  }
}

// what compute() keeps to itself, through the same public members in the same order: [convertPointsToVoxels,] normals,
// initialSegmentation, refineSegmentation[, applyVoxelsDataToPoints] -- partition uint32 [n] of the POINTS; -> the voxel count (n without voxels)
extern "C" long krs_partition( const int16_t* xyz, const uint8_t* rgb, size_t n, const int32_t* ip, const double* dp, int voxDim, uint32_t* partition ) {
  Hush         hush;
  PCCPointSet3 cloud, voxelCloud;
  cloudOf( cloud, xyz, rgb, n );
  PCCPatchSegmenter3Parameters q;
  paramsOf( q, ip, dp, voxDim != 0, voxDim );
  PCCPatchSegmenter3 segmenter;
  segmenter.setNbThread( 1 );
  Voxels voxels;
  if ( voxDim )
    segmenter.convertPointsToVoxels( cloud, q.geometryBitDepth3D_, q.voxelDimensionGridBasedSegmentation_, voxelCloud, voxels );
  else
    voxelCloud = cloud;
  const long           voxelCount = long( voxelCloud.getPointCount() );
  PCCKdTree            tree( voxelCloud );
  PCCNormalsGenerator3 generator;
  const double         mx = ( std::numeric_limits<double>::max )();
  const PCCNormalsGenerator3Parameters g = {PCCVector3D( 0.0 ), mx, mx, mx, mx, q.nnNormalEstimation_, q.nnNormalEstimation_, q.nnNormalEstimation_, 0,
                                            static_cast<PCCNormalsGeneratorOrientation>( q.normalOrientation_ ), false, false, false};
  generator.compute( voxelCloud, tree, g, 1 );
  PCCVector3D planes[6];
  for ( int k = 0; k < 6; ++k ) planes[k] = PCCVector3D( 0.0 ), planes[k][k % 3] = k < 3 ? 1.0 : -1.0;
  std::vector<size_t> labels;
  segmenter.initialSegmentation( voxelCloud, generator, planes, 6, labels, q.weightNormal_ );
  segmenter.refineSegmentation( voxelCloud, tree, generator, planes, 6, q.maxNNCountRefineSegmentation_, q.lambdaRefineSegmentation_,
                                q.iterationCountRefineSegmentation_, labels );
  if ( voxDim )
    segmenter.applyVoxelsDataToPoints( n, q.geometryBitDepth3D_, q.voxelDimensionGridBasedSegmentation_, voxels, voxelCloud, generator, labels );
  for ( size_t i = 0; i < n; ++i ) partition[i] = uint32_t( labels[i] );
  return voxelCount;
}
