// Stand-alone driver of the estimator profile's call plan (csrc/est_profile_plan.hpp) for tests/test_est_profile_plan_host.py,
// built with the host sanitizers.  Every line of standard input is one question: a command and `key=value` tokens (a missing key
// is 0).
//   shape keys: nfft t_guard n_symb n_carrier np nd bps frame_words f64 pilots_in_band descr device ctx_device
//   profile plan=0|1 <shape> f64_flag= frame0= n_points= fpp= max_chunk= points=0|1 h=none|N (N unit taps)
//           taps=none|delays,.. power= (every tap's) mmse_mode= out= bins_n= bins_lo= bins_hi= (inf / nan are read)
//                                                        -> est_profile_prelude
//   chunk   <shape> fade_taps= taps= fpp= cap= budget=   -> frames per chunk of the profile and of the study, the profile's row bytes
//   pass    <shape> k_atoms= frames=                     -> the launch shapes
//   bins    n= lo= hi= n_carrier= v=a,b,..               -> the thresholds (%a), then the bin of every v (%a is read)
// A refusal answers `refused <id> <message>`.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "../../ofdm-course_amd/csrc/est_profile_plan.hpp"

using namespace ofdm;

static const char* const IDS[EST_PROFILE_REFUSALS] = {
    "ok", "args", "device", "precision", "no_data", "pilots", "nfft", "stream", "modes", "sc_ref", "channel", "tap_delay",
    "tap_count", "fade_count", "fade_missing", "fade_delay", "fade_twice", "fade_power", "register", "descr_needed",
    "descr_unwanted", "points_missing", "points_many", "mmse_points", "mmse_fading", "chunk_cap", "mer_skip", "nmse_mp",
    "both", "descr", "mmse_mode", "output", "bins"};

typedef std::map<std::string, std::string> KV;

static long long num(const KV& kv, const char* k) {
  const auto it = kv.find(k);
  return it == kv.end() ? 0 : std::atoll(it->second.c_str());
}
static double real(const KV& kv, const char* k) {
  const auto it = kv.find(k);
  return it == kv.end() ? 0.0 : std::strtod(it->second.c_str(), nullptr);
}
static std::string str(const KV& kv, const char* k, const char* dflt = "") {
  const auto it = kv.find(k);
  return it == kv.end() ? dflt : it->second;
}

static TxfShape shape(const KV& kv) {
  TxfShape s{};
  s.nfft = (int)num(kv, "nfft"); s.t_guard = (int)num(kv, "t_guard"); s.n_symb = (int)num(kv, "n_symb");
  s.n_carrier = (int)num(kv, "n_carrier"); s.np = (int)num(kv, "np"); s.nd = (int)num(kv, "nd"); s.bps = (int)num(kv, "bps");
  s.frame_words = (int)num(kv, "frame_words"); s.f64 = (int)num(kv, "f64"); s.pilots_in_band = (int)num(kv, "pilots_in_band");
  s.descr = num(kv, "descr") ? (TXF_DESCR_ON | 0x1234u) : 0u;
  s.device = (int)num(kv, "device"); s.ctx_device = (int)num(kv, "ctx_device");
  return s;
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string cmd, tok;
    in >> cmd;
    KV kv;
    while (in >> tok) {
      const size_t eq = tok.find('=');
      if (eq == std::string::npos) { std::fprintf(stderr, "bad token %s\n", tok.c_str()); return 2; }
      kv[tok.substr(0, eq)] = tok.substr(eq + 1);
    }
    const TxfShape s = shape(kv);
    if (cmd == "profile") {
      const std::string hs = str(kv, "h", "none"), ts = str(kv, "taps", "none");
      std::vector<double> h;
      std::vector<float> hf;
      if (hs != "none")
        for (long long i = 0; i < std::atoll(hs.c_str()); ++i) { h.push_back(1.0); h.push_back(0.0); hf.push_back(1.0f); hf.push_back(0.0f); }
      std::vector<int32_t> delay;
      std::vector<double> power;
      if (ts != "none") {
        std::istringstream tin(ts);
        std::string d;
        while (std::getline(tin, d, ',')) { delay.push_back((int32_t)std::atoll(d.c_str())); power.push_back(real(kv, "power")); }
      }
      const std::vector<double> snr(1, 20.0);
      const std::vector<uint64_t> seeds(1, 1);
      TxfCall c("estimator_profile", num(kv, "frame0"), num(kv, "fpp"), nullptr);
      c.plan = num(kv, "plan") ? &s : nullptr;
      c.f64_flag = num(kv, "f64_flag") != 0;
      const bool points = num(kv, "points") != 0;
      c.with_points(points ? snr.data() : nullptr, points ? seeds.data() : nullptr, num(kv, "n_points"), num(kv, "max_chunk"));
      c.with_imp(0, 0);
      const bool fading = ts != "none";
      const void* hp = hs == "none" ? nullptr : s.f64 ? (const void*)h.data() : (const void*)hf.data();
      if (fading) c.with_fading(delay.data(), power.data(), (int)delay.size());
      else c.with_h(hp, (int)(h.size() / 2));
      EstWanted e;
      e.mmse_mode = (int)num(kv, "mmse_mode");
      e.out = num(kv, "out") != 0;
      HestBins b;
      b.n = (int)num(kv, "bins_n"); b.lo = real(kv, "bins_lo"); b.hi = real(kv, "bins_hi");
      TxfChannel ch;
      TxfGains g;
      TxfWhy w;
      const int id = est_profile_prelude(c, fading && hs != "none", e, b, ch, g, w);
      if (id < 0 || id >= EST_PROFILE_REFUSALS) { std::fprintf(stderr, "bad id %d\n", id); return 3; }
      if (id != TXF_OK) std::printf("refused %s %s\n", IDS[id], w.text);
      else std::printf("ok\n");
    } else if (cmd == "chunk") {
      const TxfUse u = txf_study_use(false, false, (int)num(kv, "fade_taps"));
      const int taps = (int)num(kv, "taps");
      const size_t budget = num(kv, "budget") ? (size_t)num(kv, "budget") : 2 * TXF_WS_BUDGET;
      std::printf("%lld %lld %zu\n", (long long)est_profile_chunk(s, u, taps, num(kv, "fpp"), num(kv, "cap"), budget),
                  (long long)est_chunk(s, u, taps, num(kv, "fpp"), num(kv, "cap"), budget), est_profile_row_bytes(s, taps));
    } else if (cmd == "pass") {
      const EstProfilePass p = est_profile_pass(s, (int)num(kv, "k_atoms"), num(kv, "frames"));
      std::printf("%d %u %u %zu %d %u %zu %d %u\n", p.acc_threads, p.acc_grid, p.acc_quantities, p.acc_lds, p.delay_threads, p.delay_grid,
                  p.delay_lds, p.hist_threads, p.hist_grid);
    } else if (cmd == "bins") {
      HestBins b;
      b.n = (int)num(kv, "n"); b.lo = real(kv, "lo"); b.hi = real(kv, "hi");
      std::vector<double> thr((size_t)b.n + 1);
      hest_thresholds(b, (int)num(kv, "n_carrier"), thr.data());
      for (double t : thr) std::printf("%a ", t);
      std::printf("|");
      std::istringstream vin(str(kv, "v"));
      std::string v;
      while (std::getline(vin, v, ',')) std::printf(" %d", hest_bin(std::strtod(v.c_str(), nullptr), thr.data(), b.n));
      std::printf("\n");
    } else {
      std::fprintf(stderr, "unknown command %s\n", cmd.c_str());
      return 2;
    }
  }
  return 0;
}
