// Stand-alone driver of the host builder of the MMSE (h = ifft(H_LS)) moment forms, for tests/test_mmse_ls_host.py: built on its
// own (with the address and undefined-behaviour sanitizers) and run as a program, no device and no library behind it.
//   mmse_ls_forms_main <N_carrier> <Np> <W.bin> <A.bin>
// W.bin: the interpolate operator [N_carrier x Np], column-major doubles; A.bin: A_q [3][Np][Np] complex doubles (A_q(i, j) at
// q Np^2 + j Np + i).
#include <cstdio>
#include <cstdlib>

#include "../ofdm-course_amd/csrc/mmse_ls_forms.hpp"

int main(int argc, char** argv) {
  if (argc != 5) { std::fprintf(stderr, "usage: %s N_carrier Np W.bin A.bin\n", argv[0]); return 2; }
  const int nc = std::atoi(argv[1]), np = std::atoi(argv[2]);
  if (nc < 1 || np < 1) { std::fprintf(stderr, "bad sizes\n"); return 2; }
  std::vector<double> W((size_t)nc * np);
  std::FILE* fi = std::fopen(argv[3], "rb");
  if (!fi || std::fread(W.data(), sizeof(double), W.size(), fi) != W.size()) { std::fprintf(stderr, "cannot read %s\n", argv[3]); return 1; }
  std::fclose(fi);
  std::vector<ofdm::ls_zc> A;
  ofdm::build_ls_moment_forms(W.data(), nc, np, A);
  std::FILE* fo = std::fopen(argv[4], "wb");
  if (!fo || std::fwrite(A.data(), sizeof(ofdm::ls_zc), A.size(), fo) != A.size()) { std::fprintf(stderr, "cannot write %s\n", argv[4]); return 1; }
  std::fclose(fo);
  return 0;
}
