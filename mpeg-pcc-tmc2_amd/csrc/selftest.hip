// selftest.hip -- the shared device primitives, each reachable on its own through the C ABI (include/tmc2hip.h: tmc2_selftest_*),
// so that the suite can compare them with a plain loop at shapes no test cloud produces: exclusiveScanU32 and fillRegions
// (scan.hip), the XCD work mapping (internal.h), UnionFind<false / true> (union_find.h), CandSort (cand_sort.h), the marked
// cells of a boundary-cell grid (cell_grid.h, cell_grid.hip; this one waits for its count, as the stages do) and the cross-lane
// idioms of wave.h.  The entries take DEVICE pointers and queue on the context's stream without synchronising: a test queues many
// calls, then reads back.  (tmc2_selftest_pool_probe reads a block of the context's pool as it is handed out: option POOL_POISON.)
// Nothing of the product path calls into this file.  (S7's own kernels on a caller's neighbour table: tmc2_selftest_components,
// patches.hip -- the kernels are local to that file.)
#include <algorithm>
#include <utility>

#include "cand_sort.h"
#include "cell_grid.h"
#include "internal.h"
#include "union_find.h"
#include "wave.h"

namespace tmc2 {
namespace {

constexpr uint32_t kNoBlock = 0xFFFFFFFFu;  // logical[b] of a surplus workgroup of the live-blocks form

// One lane, one element, found with the helpers of internal.h only.  hits[0][i]: chunkedIndex() (live: knnKernel's form, perXcd
// from the live count, surplus slots leave); hits[1][i]: pointOfLane().  logical[b]: the logical block of workgroup b.
__global__ void workMapKernel( uint32_t n, uint32_t liveBlocks, uint32_t* __restrict__ hits, uint32_t* __restrict__ logical ) {
  if ( liveBlocks ) {
    const uint32_t perXcd = ( liveBlocks + 7u ) >> 3;
    if ( xcdPlace().slot >= perXcd ) {
      if ( threadIdx.x == 0 ) logical[blockIdx.x] = kNoBlock;
      return;
    }
    const uint32_t block = chunkedBlock( perXcd ), j = block * blockDim.x + threadIdx.x;
    if ( threadIdx.x == 0 ) logical[blockIdx.x] = block;
    if ( j < n ) atomicAdd( &hits[j], 1u ), atomicAdd( &hits[size_t( n ) + j], 1u );
    return;
  }
  const bool chunked = !( gridDim.x & 7u );
  if ( threadIdx.x == 0 ) logical[blockIdx.x] = logicalBlock( chunked );
  const uint32_t a = chunkedIndex(), b = pointOfLane( nullptr, chunked, n );
  if ( a < n ) atomicAdd( &hits[a], 1u );
  if ( b < n ) atomicAdd( &hits[size_t( n ) + b], 1u );
}

// ---- union-find over an explicit edge list (a, b, s): what a 16-NN table cannot hold (a hub of 99 999 leaves, one edge 4 096 times)
template <bool PARITY>
__global__ __launch_bounds__( 256 ) void ufEdgesKernel( uint32_t* word, uint32_t n, const uint32_t* __restrict__ edges, uint32_t m,
                                                         int precheck, bool agent ) {
  const uint32_t e = chunkedIndex();
  if ( e >= m ) return;
  const uint32_t a = edges[3 * size_t( e )], b = edges[3 * size_t( e ) + 1], s = edges[3 * size_t( e ) + 2] & 1u;
  if ( a >= n || b >= n ) return;  // (counted by ufCoherentKernel)
  if ( precheck && UnionFind<PARITY>::sameSetStale( word, a, b, agent ) ) return;
  UnionFind<PARITY>::unite( word, a, b, s, agent );
}
// (the flat view goes to arrays of its own: union_find.h)
template <bool PARITY>
__global__ __launch_bounds__( 256 ) void ufFindKernel( uint32_t* word, uint32_t n, bool agent, uint32_t* __restrict__ root,
                                                        uint32_t* __restrict__ rootParity ) {
  const uint32_t x = chunkedIndex();
  if ( x >= n ) return;
  const UfRoot r = UnionFind<PARITY>::find( word, x, agent );
  root[x]        = r.root;
  rootParity[x]  = r.parity;
}
// bad[0]: elements whose climb meets a link that does not fall in priority or leaves [0, n), and edges with an end outside [0, n);
// bad[1]: edges whose ends have two roots
template <bool PARITY>
__global__ __launch_bounds__( 256 ) void ufCoherentKernel( const uint32_t* word, uint32_t n, const uint32_t* __restrict__ edges, uint32_t m,
                                                            uint32_t* __restrict__ bad ) {
  const uint32_t x = chunkedIndex();
  if ( x < n && UnionFind<PARITY>::rootCoherent( word, x, n ) == kUfBroken ) atomicAdd( &bad[0], 1u );
  if ( x < m ) {
    const uint32_t a = edges[3 * size_t( x )], b = edges[3 * size_t( x ) + 1];
    if ( a >= n || b >= n ) {
      atomicAdd( &bad[0], 1u );
      return;
    }
    const uint32_t ra = UnionFind<PARITY>::rootCoherent( word, a, n ), rb = UnionFind<PARITY>::rootCoherent( word, b, n );
    if ( ra != kUfBroken && rb != kUfBroken && ra != rb ) atomicAdd( &bad[1], 1u );
  }
}

// ---- CandSort::sort, one list per lane, as the colour transfers run it
__global__ __launch_bounds__( 256 ) void candSortKernel( uint2* __restrict__ lists, const uint32_t* __restrict__ offsets, uint32_t count,
                                                          uint32_t* __restrict__ ok ) {
  const uint32_t l = blockIdx.x * blockDim.x + threadIdx.x;
  if ( l >= count ) return;
  const CandSort cs{lists + offsets[l]};
  ok[l] = cs.sort( int( offsets[l + 1] - offsets[l] ) ) ? 1u : 0u;
}

// ---- slotOfKey of a caller's keys (a key beyond the grid: not marked)
__global__ __launch_bounds__( 256 ) void slotOfKeysKernel( const uint32_t* __restrict__ bits, const uint32_t* __restrict__ rank, uint32_t cells,
                                                            const uint32_t* __restrict__ keys, uint32_t count, uint32_t* __restrict__ slots ) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if ( k < count ) slots[k] = keys[k] < cells ? slotOfKey( bits, rank, keys[k] ) : kNoSlot;
}

// ---- wave.h, one primitive per launch (the op codes of tmc2_selftest_wave)
enum WaveOp { kWaveScan, kWaveScan16, kWaveSum, kWaveSum16, kWaveMin, kWaveMax, kWaveCompact, kWaveSort, kWaveBlockScan };

// out[i] = the primitive's value on lane i; workgroups of 256: four wavefronts with data of their own
template <int OP, typename T>
__global__ __launch_bounds__( 256 ) void waveLaneKernel( const T* __restrict__ in, T* __restrict__ out ) {
  const uint32_t i    = blockIdx.x * 256 + threadIdx.x;
  const int      lane = threadIdx.x & 63;
  const T        v    = in[i];
  if constexpr ( OP == kWaveScan ) out[i] = waveInclusive( v, lane );
  if constexpr ( OP == kWaveScan16 ) out[i] = waveInclusive<16>( v, lane );
  if constexpr ( OP == kWaveSum ) out[i] = waveSum( v );
  if constexpr ( OP == kWaveSum16 ) out[i] = waveSum<16>( v );
  if constexpr ( OP == kWaveMin ) out[i] = waveMin( v );
  if constexpr ( OP == kWaveMax ) out[i] = waveMax( v );
}
template <typename T>
void waveLaneLaunch( int op, uint32_t blocks, hipStream_t s, const void* d_in, void* d_out ) {
  const T* in  = static_cast<const T*>( d_in );
  T*       out = static_cast<T*>( d_out );
  switch ( op ) {
    case kWaveScan: hipLaunchKernelGGL( ( waveLaneKernel<kWaveScan, T> ), dim3( blocks ), dim3( 256 ), 0, s, in, out ); break;
    case kWaveScan16: hipLaunchKernelGGL( ( waveLaneKernel<kWaveScan16, T> ), dim3( blocks ), dim3( 256 ), 0, s, in, out ); break;
    case kWaveSum: hipLaunchKernelGGL( ( waveLaneKernel<kWaveSum, T> ), dim3( blocks ), dim3( 256 ), 0, s, in, out ); break;
    case kWaveSum16: hipLaunchKernelGGL( ( waveLaneKernel<kWaveSum16, T> ), dim3( blocks ), dim3( 256 ), 0, s, in, out ); break;
    case kWaveMin: hipLaunchKernelGGL( ( waveLaneKernel<kWaveMin, T> ), dim3( blocks ), dim3( 256 ), 0, s, in, out ); break;
    default: hipLaunchKernelGGL( ( waveLaneKernel<kWaveMax, T> ), dim3( blocks ), dim3( 256 ), 0, s, in, out ); break;
  }
}
// laneRank through a stream compaction: a wavefront's lanes with in != 0 write their lane number back to back from the wavefront's
// first slot on (the other slots: 0xFFFFFFFF); aux[i] = the wavefront's count
__global__ __launch_bounds__( 256 ) void waveCompactKernel( const uint32_t* __restrict__ in, uint32_t* __restrict__ out, uint32_t* __restrict__ aux ) {
  __shared__ uint32_t slots[256];
  const uint32_t i    = blockIdx.x * 256 + threadIdx.x;
  const int      lane = threadIdx.x & 63;
  const bool     mine = in[i] != 0;
  slots[threadIdx.x]  = 0xFFFFFFFFu;
  __builtin_amdgcn_fence( __ATOMIC_ACQ_REL, "wavefront" );
  const unsigned long long m = __ballot( mine );
  if ( mine ) slots[( threadIdx.x & ~63u ) + laneRank( m, lane )] = uint32_t( lane );
  __builtin_amdgcn_fence( __ATOMIC_ACQ_REL, "wavefront" );
  out[i] = slots[threadIdx.x];
  aux[i] = uint32_t( __popcll( m ) );
}
// one wavefront per list of P keys
__global__ __launch_bounds__( 64 ) void waveSortKernel( const uint32_t* __restrict__ in, uint32_t* __restrict__ out, int P ) {
  extern __shared__ uint32_t sortKeys[];
  const int    lane = threadIdx.x;
  const size_t base = size_t( blockIdx.x ) * P;
  for ( int i = lane; i < P; i += 64 ) sortKeys[i] = in[base + i];
  __builtin_amdgcn_fence( __ATOMIC_ACQ_REL, "wavefront" );
  ldsBitonicSort( sortKeys, P, lane );
  for ( int i = lane; i < P; i += 64 ) out[base + i] = sortKeys[i];
}
// out[i] = the values before thread i in its workgroup, aux[i] = the workgroup's total as thread i has it
template <int WAVES>
__global__ __launch_bounds__( 64 * WAVES ) void waveBlockScanKernel( const uint32_t* __restrict__ in, uint32_t* __restrict__ out, uint32_t* __restrict__ aux ) {
  __shared__ uint32_t waveTot[WAVES];
  const uint32_t      i = blockIdx.x * ( 64 * WAVES ) + threadIdx.x;
  uint32_t            total;
  out[i] = blockExclusive<WAVES>( in[i], waveTot, total );
  aux[i] = total;
}

// fillRegions takes a braced list: one call shape per count
template <size_t... I>
int fillWith( tmc2_ctx* ctx, const FillRegion* r, std::index_sequence<I...> ) {
  return fillRegions( ctx, {r[I]...} );
}
template <size_t N>
int fillCount( tmc2_ctx* ctx, const FillRegion* r, size_t count ) {
  if ( count == N ) return fillWith( ctx, r, std::make_index_sequence<N>() );
  if constexpr ( N > 0 ) return fillCount<N - 1>( ctx, r, count );
  return TMC2_E_INVALID;
}
constexpr size_t kSelftestFillMax = 13;  // one more than fillRegions takes: its refusal is reachable

template <bool PARITY>
int unionFindEdges( tmc2_ctx* ctx, uint32_t* d_word, uint32_t n, const uint32_t* d_edges, uint32_t m, int precheck, bool agent,
                    uint32_t* d_root, uint32_t* d_rootParity, uint32_t* d_bad ) {
  hipStream_t s = ctx->stream;
  const dim3  blk( 256 ), grdN( chunkedGrid( ( n + 255 ) / 256 ) ), grdM( chunkedGrid( ( m + 255 ) / 256 ) ),
      grdBoth( chunkedGrid( ( std::max( n, m ) + 255 ) / 256 ) );
  if ( m ) hipLaunchKernelGGL( ufEdgesKernel<PARITY>, grdM, blk, 0, s, d_word, n, d_edges, m, precheck, agent );
  hipLaunchKernelGGL( ufFindKernel<PARITY>, grdN, blk, 0, s, d_word, n, agent, d_root, d_rootParity );
  hipLaunchKernelGGL( ufCoherentKernel<PARITY>, grdBoth, blk, 0, s, d_word, n, d_edges, m, d_bad );
  TMC2_HIP( hipGetLastError() );
  return TMC2_OK;
}

}  // namespace
}  // namespace tmc2

extern "C" {

int tmc2_selftest_scan( tmc2_ctx* ctx, const uint32_t* d_in, uint32_t* d_out, uint64_t n, uint32_t* d_total, uint32_t* hostAnswer,
                        const uint32_t* d_carry, int carryWords, uint64_t epoch ) {
  using namespace tmc2;
  if ( !ctx || ( n && ( !d_in || !d_out ) ) || carryWords < 0 || carryWords > 7 || ( carryWords && ( !hostAnswer || !d_carry ) ) ||
       epoch > 0x3FFFFFFFull ) {
    setError( "selftest_scan: invalid argument (null pointer, more than 7 carry words, carry words without an answer line, or an epoch beyond 30 bits)" );
    return TMC2_E_INVALID;
  }
  ApiScope scope( ctx );
  if ( epoch ) ctx->scanEpoch = uint32_t( epoch );  // the one back door: the wrap is 2^30 scans away otherwise
  return exclusiveScanU32( ctx, d_in, d_out, size_t( n ), d_total, ScanAnswer{hostAnswer, d_carry, carryWords} );
}

int tmc2_selftest_fill( tmc2_ctx* ctx, const uint64_t* regions, int count ) {
  using namespace tmc2;
  if ( !ctx || count < 0 || count > int( kSelftestFillMax ) || ( count && !regions ) ) {
    setError( "selftest_fill: invalid argument (null pointer or more than %d regions)", int( kSelftestFillMax ) );
    return TMC2_E_INVALID;
  }
  FillRegion r[kSelftestFillMax] = {};
  for ( int k = 0; k < count; ++k ) {
    if ( regions[3 * k + 1] && !regions[3 * k] ) {
      setError( "selftest_fill: region %d has bytes and no address", k );
      return TMC2_E_INVALID;
    }
    r[k] = FillRegion{reinterpret_cast<void*>( uintptr_t( regions[3 * k] ) ), size_t( regions[3 * k + 1] ), uint8_t( regions[3 * k + 2] )};
  }
  ApiScope scope( ctx );
  return fillCount<kSelftestFillMax>( ctx, r, size_t( count ) );
}

int tmc2_selftest_work_map( tmc2_ctx* ctx, uint64_t gridBlocks, int blockThreads, uint64_t n, uint64_t liveBlocks, uint32_t* d_hits,
                            uint32_t* d_logical ) {
  using namespace tmc2;
  if ( !ctx || !d_hits || !d_logical || blockThreads < 1 || blockThreads > 1024 || n > 0x7FFFFFFFull || gridBlocks > ( 1u << 20 ) ) {
    setError( "selftest_work_map: invalid argument (null pointer, 1 .. 1024 threads, at most 2^20 blocks and 2^31 - 1 elements)" );
    return TMC2_E_INVALID;
  }
  // no grid given: the grid a stage gives a chunked pass over n elements
  const uint32_t grid = gridBlocks ? uint32_t( gridBlocks ) : chunkedGrid( uint32_t( ( n + uint64_t( blockThreads ) - 1 ) / uint64_t( blockThreads ) ) );
  if ( grid == 0 || ( liveBlocks && ( ( grid & 7u ) || liveBlocks > grid ) ) ) {
    setError( "selftest_work_map: an empty grid, or live blocks on a grid that is no multiple of 8 or smaller than their number" );
    return TMC2_E_INVALID;
  }
  ApiScope scope( ctx );
  hipLaunchKernelGGL( workMapKernel, dim3( grid ), dim3( uint32_t( blockThreads ) ), 0, ctx->stream, uint32_t( n ), uint32_t( liveBlocks ), d_hits,
                      d_logical );
  TMC2_HIP( hipGetLastError() );
  return TMC2_OK;
}

int tmc2_selftest_union_find( tmc2_ctx* ctx, int parity, uint32_t* d_word, uint64_t n, const uint32_t* d_edges, uint64_t m, int precheck,
                              int agent, uint32_t* d_root, uint32_t* d_rootParity, uint32_t* d_bad ) {
  using namespace tmc2;
  if ( !ctx || !d_word || !d_root || !d_rootParity || !d_bad || n == 0 || n > 0x7FFFFFFFull || m > 0x7FFFFFFFull || ( m && !d_edges ) ) {
    setError( "selftest_union_find: invalid argument (null pointer, no element, or more than 2^31 - 1 elements or edges)" );
    return TMC2_E_INVALID;
  }
  ApiScope scope( ctx );
  return parity ? unionFindEdges<true>( ctx, d_word, uint32_t( n ), d_edges, uint32_t( m ), precheck, agent != 0, d_root, d_rootParity, d_bad )
                : unionFindEdges<false>( ctx, d_word, uint32_t( n ), d_edges, uint32_t( m ), precheck, agent != 0, d_root, d_rootParity, d_bad );
}

int tmc2_selftest_cand_sort( tmc2_ctx* ctx, uint32_t* d_lists, const uint32_t* d_offsets, uint64_t lists, uint32_t* d_ok ) {
  using namespace tmc2;
  if ( !ctx || !d_lists || !d_offsets || !d_ok || lists == 0 || lists > 0x7FFFFFFFull ) {
    setError( "selftest_cand_sort: invalid argument (null pointer, no list, or more than 2^31 - 1 lists)" );
    return TMC2_E_INVALID;
  }
  ApiScope scope( ctx );
  hipLaunchKernelGGL( candSortKernel, dim3( uint32_t( ( lists + 255 ) / 256 ) ), dim3( 256 ), 0, ctx->stream, reinterpret_cast<uint2*>( d_lists ),
                      d_offsets, uint32_t( lists ), d_ok );
  TMC2_HIP( hipGetLastError() );
  return TMC2_OK;
}

int tmc2_selftest_marked_cells( tmc2_ctx* ctx, const int16_t* d_xyz4, const uint8_t* d_boundaryType, uint64_t M, int gridSize, int bits,
                                int maxCoord, uint32_t* cells, uint32_t* d_bits, uint32_t* d_rank, const uint32_t* d_keys, uint64_t keys,
                                uint32_t* d_slots ) {
  using namespace tmc2;
  if ( !ctx || !cells || ( M && ( !d_xyz4 || !d_boundaryType ) ) || M > 0x7FFFFFFFull || keys > 0x7FFFFFFFull || ( keys && ( !d_keys || !d_slots ) ) ||
       gridSize < 2 || gridSize > 64 || ( gridSize & 1 ) || bits < 0 || bits > 14 || maxCoord < 0 || maxCoord > 32767 ) {
    // (an odd gridSize: the upper cell of a point in the last cell before a face lies outside the grid)
    setError( "selftest_marked_cells: invalid argument (null pointer, gridSize not even or outside 2 .. 64, bits beyond 14, maxCoord beyond 32767)" );
    return TMC2_E_INVALID;
  }
  const CellGrid g = bits ? cubeCellGrid( gridSize, bits ) : extentCellGrid( gridSize, maxCoord );
  if ( g.cells() == 0 || g.cells() > ( uint64_t( 1 ) << 31 ) ) {
    setError( "selftest_marked_cells: a grid of %d^3 cells", g.w );
    return TMC2_E_INVALID;
  }
  ApiScope         scope( ctx );
  hipStream_t      s = ctx->stream;
  MarkedCells      marked;
  DevBuf<uint32_t> d_total;
  TMC2_TRY( d_total.alloc( 1 ) );
  TMC2_TRY( markedCells( ctx, reinterpret_cast<const Pt*>( d_xyz4 ), d_boundaryType, uint32_t( M ), g, d_total.p, marked ) );
  *cells = marked.count;
  if ( d_bits ) TMC2_HIP( hipMemcpyAsync( d_bits, marked.bits.p, size_t( marked.words ) * 4, hipMemcpyDeviceToDevice, s ) );
  if ( d_rank ) TMC2_HIP( hipMemcpyAsync( d_rank, marked.rank.p, size_t( marked.words ) * 4, hipMemcpyDeviceToDevice, s ) );
  if ( keys )
    hipLaunchKernelGGL( slotOfKeysKernel, dim3( uint32_t( ( keys + 255 ) / 256 ) ), dim3( 256 ), 0, s, marked.bits.p, marked.rank.p,
                        uint32_t( g.cells() ), d_keys, uint32_t( keys ), d_slots );
  TMC2_HIP( hipStreamSynchronize( s ) );  // (the bit words and ranks go back to the pool with `marked`)
  TMC2_HIP( hipGetLastError() );
  return TMC2_OK;
}

int tmc2_selftest_wave( tmc2_ctx* ctx, int op, int param, const void* d_in, void* d_out, uint32_t* d_aux, uint64_t n ) {
  using namespace tmc2;
  const bool     perLane = op >= kWaveScan && op <= kWaveMax;
  const bool     sizeOk  = op == kWaveSort        ? param >= 64 && param <= 8192 && !( param & ( param - 1 ) )
                           : op == kWaveBlockScan ? param == 1 || param == 2 || param == 4 || param == 16
                                                  : !perLane || ( param >= 0 && param <= 2 );
  const uint64_t group   = op == kWaveSort ? uint64_t( param ) : op == kWaveBlockScan ? 64u * uint64_t( param ) : 256u;
  if ( !ctx || !d_in || !d_out || op < kWaveScan || op > kWaveBlockScan || !sizeOk || n == 0 || n > ( 1u << 24 ) || n % group ||
       ( ( op == kWaveCompact || op == kWaveBlockScan ) && !d_aux ) ) {
    setError( "selftest_wave: invalid argument (null pointer, unknown op, a type beyond 2, a sort length that is no power of two in 64 .. 8192, "
              "a workgroup of other than 1, 2, 4 or 16 wavefronts, no element, more than 2^24, or no whole number of groups)" );
    return TMC2_E_INVALID;
  }
  ApiScope        scope( ctx );
  hipStream_t     s      = ctx->stream;
  const uint32_t  blocks = uint32_t( n / group );
  const uint32_t* in     = static_cast<const uint32_t*>( d_in );
  uint32_t*       out    = static_cast<uint32_t*>( d_out );
  if ( perLane ) {
    if ( param == 0 ) waveLaneLaunch<uint32_t>( op, blocks, s, d_in, d_out );
    if ( param == 1 ) waveLaneLaunch<int>( op, blocks, s, d_in, d_out );
    if ( param == 2 ) waveLaneLaunch<double>( op, blocks, s, d_in, d_out );
  } else if ( op == kWaveCompact ) {
    hipLaunchKernelGGL( waveCompactKernel, dim3( blocks ), dim3( 256 ), 0, s, in, out, d_aux );
  } else if ( op == kWaveSort ) {
    hipLaunchKernelGGL( waveSortKernel, dim3( blocks ), dim3( 64 ), size_t( param ) * 4, s, in, out, param );
  } else {
    if ( param == 1 ) hipLaunchKernelGGL( waveBlockScanKernel<1>, dim3( blocks ), dim3( 64 ), 0, s, in, out, d_aux );
    if ( param == 2 ) hipLaunchKernelGGL( waveBlockScanKernel<2>, dim3( blocks ), dim3( 128 ), 0, s, in, out, d_aux );
    if ( param == 4 ) hipLaunchKernelGGL( waveBlockScanKernel<4>, dim3( blocks ), dim3( 256 ), 0, s, in, out, d_aux );
    if ( param == 16 ) hipLaunchKernelGGL( waveBlockScanKernel<16>, dim3( blocks ), dim3( 1024 ), 0, s, in, out, d_aux );
  }
  TMC2_HIP( hipGetLastError() );
  return TMC2_OK;
}

// A block of the context's pool as acquire hands it out, read without having been written -- on purpose: under option POOL_POISON
// every byte of the size class is the poison byte; without it the content is whatever the last owner or the driver left.
// hostOut null: only the size class is reported.  This one waits: the block goes back to the pool when it returns.
int tmc2_selftest_pool_probe( tmc2_ctx* ctx, uint64_t bytes, uint8_t* hostOut, uint64_t* classBytes ) {
  using namespace tmc2;
  if ( !ctx || !classBytes || bytes == 0 || bytes > ( uint64_t( 1 ) << 30 ) ) {
    setError( "selftest_pool_probe: invalid argument (null pointer, no byte or more than 2^30)" );
    return TMC2_E_INVALID;
  }
  *classBytes = DevicePool::sizeClass( size_t( bytes ) );
  if ( !hostOut ) return TMC2_OK;
  ApiScope        scope( ctx );
  DevBuf<uint8_t> block;
  TMC2_TRY( block.alloc( size_t( bytes ) ) );
  if ( block.bytes() != *classBytes ) {
    setError( "selftest_pool_probe: a block of %zu bytes for the class of %llu", block.bytes(), static_cast<unsigned long long>( *classBytes ) );
    return TMC2_E_HIP;
  }
  TMC2_HIP( hipMemcpyAsync( hostOut, block.p, block.bytes(), hipMemcpyDeviceToHost, ctx->stream ) );
  TMC2_HIP( hipStreamSynchronize( ctx->stream ) );
  return TMC2_OK;
}
// how many blocks the context's pool has filled with the poison byte so far
int tmc2_selftest_pool_poisoned( tmc2_ctx* ctx, uint64_t* blocks ) {
  if ( !ctx || !blocks ) {
    tmc2::setError( "selftest_pool_poisoned: invalid argument" );
    return TMC2_E_INVALID;
  }
  std::lock_guard<std::mutex> g( ctx->pool.lock );
  *blocks = ctx->pool.poisonedBlocks;
  return TMC2_OK;
}

// the host twin: the real std::sort with the reference's comparator, on host memory
int tmc2_selftest_std_sort( uint32_t* lists, const uint32_t* offsets, uint64_t count ) {
  if ( !lists || !offsets ) {
    tmc2::setError( "selftest_std_sort: invalid argument" );
    return TMC2_E_INVALID;
  }
  struct Cand {
    uint32_t dist, index;
  };
  Cand* c = reinterpret_cast<Cand*>( lists );
  for ( uint64_t l = 0; l < count; ++l ) {
    if ( offsets[l + 1] < offsets[l] ) {
      tmc2::setError( "selftest_std_sort: offsets fall at list %llu", static_cast<unsigned long long>( l ) );
      return TMC2_E_INVALID;
    }
    std::sort( c + offsets[l], c + offsets[l + 1], []( const Cand& a, const Cand& b ) { return a.dist < b.dist; } );
  }
  return TMC2_OK;
}

}  // extern "C"
