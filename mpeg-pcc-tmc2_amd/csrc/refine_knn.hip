// refine_knn.hip -- the refinement of the segmentation over k-NN neighbourhoods (the reference's non-grid mode) on gfx950.
//
// Replaces PCCPatchSegmenter3::refineSegmentation (PccLibEncoder/source/PCCPatchSegmenter.cpp:1322-1384).  The branch of
// PCCPatchSegmenter3::compute that calls it (:126-131), with gridBasedSegmentation_ or without, is segmenterCompute's
// (segmenter_api.cpp: the one chain of the segmenter's modes).
//
// The neighbourhoods come from the wide search (knn_wide.hip) as TREE POSITIONS in the layout adj[e][j], j = the point's own tree
// position: one point per lane, so the 64 lanes of a wave read 64 consecutive words per step, and the partition bytes they gather
// are those of tree-order neighbours -- the eighth of the cloud an XCD works on (internal.h: the XCD work mapping) stays in its
// L2.  The partition is one byte per point, in tree order, in two buffers (Jacobi: a round reads one and writes the other); the
// six counters of a point are five 12-bit fields of one 64-bit register and K minus their sum.  The vote is refine_knn.h's.
//
// Early exit without a host round trip: four device words.  state[r % 3] collects "some point changed its plane in round r";
// round r starts by reading state[( r - 1 ) % 3] -- zero: round r - 1 changed nothing (or did not run), a round is a function of
// the partition alone, so this and every later launch leaves at once -- and clears state[( r + 1 ) % 3] for the next round.  Both
// buffers hold the fixed point then, whichever the last launch would have written.  A period-2 state changes points in every
// round and never ends the loop early.  state[3] counts the rounds that ran.
//
// The adjacency (n x K x 4 bytes: 853 MB for a longdress frame at K = 256) is scratch of the context, grown on demand and kept.
#include "internal.h"
#include "refine_knn.h"

namespace tmc2 {
namespace {

// tree order <- input order
__global__ __launch_bounds__( 256 ) void gatherPartitionKernel( const uint8_t* __restrict__ partition, const uint32_t* __restrict__ perm, uint32_t n,
                                                                 uint8_t* __restrict__ treePartition ) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if ( j < n ) {
    const uint8_t plane = partition[perm[j]];
    treePartition[j]    = plane < 5 ? plane : uint8_t( 5 );
  }
}
__global__ __launch_bounds__( 256 ) void scatterPartitionKernel( const uint8_t* __restrict__ treePartition, const uint32_t* __restrict__ perm, uint32_t n,
                                                                  uint8_t* __restrict__ partition ) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if ( j < n ) partition[perm[j]] = treePartition[j];
}

__global__ __launch_bounds__( 256 ) void refineKnnRoundKernel( const uint32_t* __restrict__ adj, uint32_t stride, uint32_t n, uint32_t K,
                                                                const uint32_t* __restrict__ perm, const double* __restrict__ normals,
                                                                const uint8_t* __restrict__ cur, uint8_t* __restrict__ next, double weight,
                                                                uint32_t* __restrict__ state, uint32_t round ) {
  const bool runs = round == 0 || state[( round + 2u ) % 3u] != 0u;
  if ( blockIdx.x == 0 && threadIdx.x == 0 ) {
    state[( round + 1u ) % 3u] = 0u;  // (nobody reads or writes this word during round `round`)
    if ( runs ) state[3] = state[3] + 1u;
  }
  if ( !runs ) return;
  const uint32_t j = chunkedIndex();
  if ( j >= n ) return;
  unsigned long long fields = 0ull;  // counters of planes 0..4, 12 bits each (K <= 1024)
  const uint32_t*    column = adj + j;
#pragma unroll 4
  for ( uint32_t e = 0; e < K; ++e ) {
    const uint32_t plane = cur[column[size_t( e ) * stride]];
    fields += plane < 5u ? 1ull << ( 12u * plane ) : 0ull;
  }
  uint32_t count[6], sum = 0;
  for ( int p = 0; p < 5; ++p ) count[p] = uint32_t( fields >> ( 12 * p ) ) & 0xFFFu, sum += count[p];
  count[5] = K - sum;
  const uint32_t own = cur[j];
  const size_t   i   = perm[j];
  const uint32_t to  = refineVote( normals[3 * i], normals[3 * i + 1], normals[3 * i + 2], own, count, weight );
  next[j]            = uint8_t( to );
  const unsigned long long moved = __ballot( to != own );  // one atomic per wave
  if ( moved && ( threadIdx.x & 63u ) == uint32_t( __ffsll( moved ) - 1 ) ) atomicOr( &state[round % 3u], 1u );
}

}  // namespace

int refineKnnCheck( const char* who, int maxNNCount, double lambda, int iterationCount ) {
  int offending = 0;
  if ( const char* why = refineKnnRefusal( maxNNCount, lambda, iterationCount, &offending ) ) {
    char text[192];
    snprintf( text, sizeof( text ), why, offending );
    setError( "%s: %s", who, text );
    return TMC2_E_UNSUPPORTED;
  }
  return TMC2_OK;
}

int refineKnn( tmc2_frame* f, int maxNNCount, double lambda, int iterationCount ) {
  tmc2_ctx*   ctx = f->ctx;
  hipStream_t s   = ctx->stream;
  // ---- refused before anything is launched: the frame stays as it is
  TMC2_TRY( refineKnnCheck( "segmenter_refine", maxNNCount, lambda, iterationCount ) );
  if ( !f->haveNormals || !f->havePartition || f->n == 0 || f->n > 0x7FFFFFF0ull ) {
    setError( "segmenter_refine: the frame has no normals / partition" );
    return TMC2_E_STATE;
  }
  if ( uint64_t( maxNNCount ) > f->n ) {
    setError( "segmenter_refine: maxNNCountRefineSegmentation %d larger than the cloud (%llu points)", maxNNCount, (unsigned long long)f->n );
    return TMC2_E_UNSUPPORTED;
  }
  if ( iterationCount == 0 ) return TMC2_OK;  // (the reference builds its lists and uses none)
  TMC2_TRY( f->ensureTree() );
  const uint32_t n = uint32_t( f->n ), K = uint32_t( maxNNCount ), stride = ( n + 63u ) & ~63u;
  TMC2_TRY( ctx->knnWideAdj.alloc( size_t( K ) * stride ) );
  TMC2_TRY( launchKnnWide( ctx, f->tree.view( QueryBox::Any ), nullptr, n, maxNNCount, ctx->knnWideAdj.p, true, stride ) );
  DevBuf<uint8_t>  d_a, d_b;
  DevBuf<uint32_t> d_state;
  TMC2_TRY( d_a.alloc( n ) );
  TMC2_TRY( d_b.alloc( n ) );
  TMC2_TRY( d_state.alloc( 4 ) );
  StageScope span( ctx, "refine_knn" );
  TMC2_HIP( hipMemsetAsync( d_state.p, 0, 4 * sizeof( uint32_t ), s ) );
  const dim3 blk( 256 ), grd( ( n + 255 ) / 256 ), chunked( chunkedGrid( ( n + 255 ) / 256 ) );
  hipLaunchKernelGGL( gatherPartitionKernel, grd, blk, 0, s, f->d_partition.p, f->tree.perm.p, n, d_a.p );
  const double weight = lambda / double( maxNNCount );
  uint8_t *    cur = d_a.p, *next = d_b.p;
  for ( int r = 0; r < iterationCount; ++r ) {
    hipLaunchKernelGGL( refineKnnRoundKernel, chunked, blk, 0, s, ctx->knnWideAdj.p, stride, n, K, f->tree.perm.p, f->d_normals.p, cur, next, weight,
                        d_state.p, uint32_t( r ) );
    std::swap( cur, next );
  }
  hipLaunchKernelGGL( scatterPartitionKernel, grd, blk, 0, s, cur, f->tree.perm.p, n, f->d_partition.p );
  TMC2_HIP( hipGetLastError() );
  return TMC2_OK;  // (the temporaries go back to the pool; what is queued on the stream runs before their next user's work)
}

}  // namespace tmc2

using namespace tmc2;

extern "C" {

int tmc2_segmenter_refine( tmc2_frame* f, int maxNNCount, double lambda, int iterationCount ) {
  if ( !f ) return TMC2_E_INVALID;
  ApiScope scope( f->ctx );
  return refineKnn( f, maxNNCount, lambda, iterationCount );
}

}  // extern "C"
