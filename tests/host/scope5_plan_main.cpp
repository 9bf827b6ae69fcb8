// Stand-alone driver of the Task-5 part of the constellation-capture plan (csrc/scope_plan.hpp: scope5_iq_check,
// scope5_density_check, the grid's place behind a symbol stage's LDS) for tests/test_scope5_plan_host.py, built with the host
// sanitizers.  Every line of standard input is one question, a word and `key=value` tokens:
//   iq first= count= decisions=                                   -> `ok`, or `refused <id> <message>`
//   density stage= lds= out= bins= half_width= skip= decisions=   -> `ok <grid offset> <stage bytes with the grid>`, or refused
//     (stage: 0 generic, 1 rx_symbols, 2 wave, 3 coop4, 4 r2, 5 eq_demap -- SYM_* of chain_route.hpp; lds: the stage's bytes
//      without a grid)
//   wave nd= n_symb=                                              -> the wave stage's bytes without a grid (scope5_stage_lds)
// Numbers are read with strtod / strtoll: inf, -inf and nan are accepted.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>

#include "../../ofdm-course_amd/csrc/scope_plan.hpp"

using namespace ofdm;

int main() {
  static const char* const IDS[SCOPE_REFUSALS] = {"ok", "iq_first", "iq_count", "iq_end", "density_out", "bins", "half_width",
                                                  "skip", "lds"};
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string what, tok;
    in >> what;
    long long first = 0, count = 0, decisions = 0, skip = 0, lds = 0;
    int out = 0, bins = 0, stage = 0, nd = 0, n_symb = 0;
    double half_width = 0.0;
    while (in >> tok) {
      const size_t eq = tok.find('=');
      if (eq == std::string::npos) { std::fprintf(stderr, "bad token %s\n", tok.c_str()); return 2; }
      const std::string k = tok.substr(0, eq), x = tok.substr(eq + 1);
      if (k == "first") first = std::strtoll(x.c_str(), nullptr, 10); else if (k == "count") count = std::strtoll(x.c_str(), nullptr, 10);
      else if (k == "decisions") decisions = std::strtoll(x.c_str(), nullptr, 10); else if (k == "skip") skip = std::strtoll(x.c_str(), nullptr, 10);
      else if (k == "lds") lds = std::strtoll(x.c_str(), nullptr, 10); else if (k == "out") out = std::atoi(x.c_str());
      else if (k == "bins") bins = std::atoi(x.c_str()); else if (k == "stage") stage = std::atoi(x.c_str());
      else if (k == "nd") nd = std::atoi(x.c_str()); else if (k == "n_symb") n_symb = std::atoi(x.c_str());
      else if (k == "half_width") half_width = std::strtod(x.c_str(), nullptr);
      else { std::fprintf(stderr, "unknown key %s\n", k.c_str()); return 2; }
    }
    ScopeWhy why;
    if (what == "iq" || what == "density") {
      const int id = what == "iq" ? scope5_iq_check(first, count, decisions, why)
                                  : scope5_density_check(stage, (size_t)lds, bins, half_width, skip, decisions, out != 0, why);
      if (id < 0 || id >= SCOPE_REFUSALS || (id != SCOPE_OK) != (why.text[0] != 0)) { std::fprintf(stderr, "refusal %d and its reason disagree\n", id); return 3; }
      if (id != SCOPE_OK) { std::printf("refused %s %s\n", IDS[id], why.text); continue; }
      if (what == "iq") { std::printf("ok\n"); continue; }
      std::printf("ok %zu %zu\n", scope5_grid_offset((size_t)lds), scope5_lds_total((size_t)lds, bins));
    } else if (what == "wave") {
      ChainRoute r{};
      r.symbols = SYM_WAVE;
      std::printf("%zu\n", scope5_stage_lds(r, nd, n_symb));
    } else {
      std::fprintf(stderr, "unknown question %s\n", what.c_str());
      return 2;
    }
  }
  return 0;
}
