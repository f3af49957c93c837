// tools/metrics_host_sanitize.cpp -- tmc2_host_metrics_compute (csrc/metrics_host.cpp) under AddressSanitizer and
// UndefinedBehaviorSanitizer, as a program of its own: no Python, no device, no preloaded runtime.  tools/metrics_host_sanitize.sh
// writes clouds of tests/metrics_option_cases.py to files, builds this file and metrics_host.cpp with -fsanitize=address,undefined
// and runs every cloud through dropDuplicates x neighborsProc x computeHausdorff and each single flag switched off.  A refusal
// (duplicates with normals: -3; an answer that depends on the search order: -6) is an outcome like any other here; a sanitizer
// report ends the program with a non-zero status.
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <map>
#include <vector>

#include "tmc2hip.h"

namespace tmc2 {
void setError( const char*, ... ) {}  // (the library's lives in api.cpp, next to the device code)
}  // namespace tmc2

namespace {
template <typename T>
bool readArray( FILE* f, std::vector<T>& v, size_t count ) {
  v.resize( count );
  return count == 0 || std::fread( v.data(), sizeof( T ), count, f ) == count;
}
}  // namespace

// a cloud file: int64 n, m; int16 src[n][3]; uint8 srcRgb[n][3]; int16 rec[m][3]; uint8 recRgb[m][3]; double normals[n][3]
int main( int argc, char** argv ) {
  int failures = 0;
  for ( int a = 1; a < argc; ++a ) {
    FILE* f = std::fopen( argv[a], "rb" );
    int64_t size[2] = {0, 0};
    std::vector<int16_t> src, rec;
    std::vector<uint8_t> srcRgb, recRgb;
    std::vector<double>  normals;
    if ( !f || std::fread( size, sizeof( int64_t ), 2, f ) != 2 || size[0] <= 0 || size[1] <= 0 || !readArray( f, src, 3 * size_t( size[0] ) ) ||
         !readArray( f, srcRgb, 3 * size_t( size[0] ) ) || !readArray( f, rec, 3 * size_t( size[1] ) ) || !readArray( f, recRgb, 3 * size_t( size[1] ) ) ||
         !readArray( f, normals, 3 * size_t( size[0] ) ) ) {
      std::fprintf( stderr, "%s: not a cloud file\n", argv[a] );
      return 2;
    }
    std::fclose( f );
    std::map<int, int> outcomes;
    int                runs = 0;
    auto run = [&]( tmc2_metrics_params q ) {
      double  out[3 * 14];
      int64_t counts[2];
      for ( int withNormals = 0; withNormals < 2; ++withNormals ) {
        const int rc = tmc2_host_metrics_compute( src.data(), srcRgb.data(), uint64_t( size[0] ), rec.data(), recRgb.data(), uint64_t( size[1] ),
                                                  withNormals ? normals.data() : nullptr, 1023.0, &q, out, counts );
        ++outcomes[rc], ++runs;
        if ( rc != TMC2_OK && rc != TMC2_E_INVALID && rc != TMC2_E_ORDER ) ++failures;
      }
    };
    for ( int dd = 0; dd <= 2; ++dd )
      for ( int np = 0; np <= 4; ++np )
        for ( int h = 0; h <= 1; ++h ) run( tmc2_metrics_params{1, 1, 1, h, dd, np} );
    run( tmc2_metrics_params{0, 1, 1, 1, 2, 1} );
    run( tmc2_metrics_params{1, 0, 1, 1, 2, 1} );
    run( tmc2_metrics_params{1, 1, 0, 1, 2, 1} );
    std::printf( "%s: %lld / %lld points, %d runs:", argv[a], (long long)size[0], (long long)size[1], runs );
    for ( const auto& o : outcomes ) std::printf( "  rc %d x %d", o.first, o.second );
    std::printf( "\n" );
  }
  std::printf( failures ? "FAILED: %d unexpected return codes\n" : "metrics_host_sanitize: clean (%d unexpected return codes)\n", failures );
  return failures ? 1 : 0;
}
