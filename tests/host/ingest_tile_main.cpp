// The tile chooser of the fused ingestion (ingest_tile, pytemdiags_amd/csrc/launch_shapes.hpp) on its own: the header
// needs no HIP.  usage: ingest_tile_main cases.txt > tiles.txt
// One case per input line: ncol nlev ntb nf dsz ssz.  One line out per case:
//   ok tc_shift tt kw stride ppl nct ntt nwin lds
// tests/test_ingest_host.py builds it with AddressSanitizer + UBSan and holds its numpy mirror to it.
#include <cinttypes>
#include <cstdio>

#include "../../pytemdiags_amd/csrc/launch_shapes.hpp"

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  std::FILE* in = std::fopen(argv[1], "r");
  if (!in) return 3;
  long long ncol, nlev, ntb, nf, dsz, ssz;
  while (std::fscanf(in, "%lld %lld %lld %lld %lld %lld", &ncol, &nlev, &ntb, &nf, &dsz, &ssz) == 6) {
    temx::IngestTile tl{};
    size_t lds = 0;
    const bool ok = temx::ingest_tile((int64_t)ncol, (int)nlev, (int64_t)ntb, (int)nf, (size_t)dsz, (size_t)ssz, &tl, &lds);
    std::printf("%d %d %d %d %d %d %d %d %d %zu\n", ok ? 1 : 0, tl.tc_shift, tl.tt, tl.kw, tl.stride, tl.ppl, tl.nct, tl.ntt,
                tl.nwin, lds);
  }
  std::fclose(in);
  return 0;
}
