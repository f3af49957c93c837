// color_transfer_rules_check.cpp -- csrc/color_transfer_rules.h and csrc/cand_sort.h through a plain host compiler (no device code):
// tests/test_color_transfer_options_host.py compiles this with g++ and reads what it prints.  One target whose two forward
// neighbours and three backward candidates are written out here, under the CTC set and under a set with a search range.
#include <cstddef>
#include <cstdio>

#include "cand_sort.h"
#include "color_transfer_rules.h"

struct Entry {
  unsigned x, y;
};

int main() {
  using namespace tmc2;
  tmc2_color_transfer_params q;
  ctDefault( q );
  printf( "sizeof %zu\n", sizeof( q ) );
  printf( "offsets %zu %zu %zu %zu %zu\n", offsetof( tmc2_color_transfer_params, numNeighborsColorTransferFwd ),
          offsetof( tmc2_color_transfer_params, distOffsetFwd ), offsetof( tmc2_color_transfer_params, maxColorDist2Bwd ),
          offsetof( tmc2_color_transfer_params, excludeColorOutlier ), offsetof( tmc2_color_transfer_params, thresholdColorOutlierDist ) );
  printf( "default %d refusal %s\n", int( ctIsDefault( q ) ), ctRefusal( q ) ? ctRefusal( q ) : "none" );
  const unsigned dist[2]   = {1, 4};
  const CtColor  colors[3] = {{10, 20, 30}, {20, 20, 30}, {250, 0, 7}};
  q.numNeighborsColorTransferFwd = 2;
  const CtColor f = ctForward( ctRules( q ), 2, [&]( int i ) { return dist[i]; }, [&]( int i ) { return colors[i]; } );
  printf( "forward %d %d %d\n", f.c0, f.c1, f.c2 );  // ( 10 / 5 + 20 / 8 ) / ( 1 / 5 + 1 / 8 ) = 13.846..
  Entry e[3] = {{9, 2}, {1, 0}, {4, 1}};
  printf( "sorted %d\n", int( CandSortOf<Entry>{e}.sort( 3 ) ) );
  q.searchRange  = 2;
  const CtColor b = ctBackward( ctRules( q ), 3, [&]( int i ) { return e[i].x; }, [&]( int i ) { return colors[e[i].y]; }, f, 1.0 / 3.0, 1.0 / 3.0 );
  printf( "backward %d %d %d order %u %u %u\n", b.c0, b.c1, b.c2, e[0].y, e[1].y, e[2].y );
  q.distOffsetBwd = 0.0;
  printf( "refusal %s\n", ctRefusal( q ) );
  return 0;
}
