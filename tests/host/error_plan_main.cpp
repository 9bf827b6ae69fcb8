// Stand-alone driver of the error anatomy's call plan (csrc/error_plan.hpp) for tests/test_error_plan_host.py, built with the host
// sanitizers.  Every line of standard input is one question: a command and `key=value` tokens (a missing key is 0).
//   shape keys: nfft t_guard n_symb n_carrier np nd bps frame_words f64 pilots_in_band descr mmse device ctx_device
//   profile plan=0|1 <shape> bits= ref= n_frames= gap_bins= out=                      -> err_profile_prelude
//   study   plan=0|1 <shape> receiver= side= f64_flag= frame0= n_points= fpp= max_chunk= points=0|1 sto_mode= cfo_mode=
//           time_desync= freq_desync= mp_desync= reg=none|15 digits h=none|bad|N (N unit taps) taps=none|delays,.. power= (every
//           tap's) gap_bins= out=                                                     -> err_study_prelude
//   chunk   <shape> receiver= scr= fade_taps= fpp= cap=                               -> frames per chunk, bytes per frame, bit bytes
//   pass    <shape> gap_bins= frames=              -> threads symbols_in_lds lds flush_frames launch_frames grid
//   pos     nd= bps= i=                            -> s d r of stream bit i (err_position)
//   walk    nd= bps= i=                            -> for delta 0 .. 32: s d r of bit i + delta by one err_advance from bit i, then
//                                                     the same 33 positions by a chain of err_advance of one bit each
//   div     bps=                                   -> err_small_div(n, err_recip(bps)) for n = 0 .. 63
// A refusal answers `refused <id> <message>`.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "../../ofdm-course_amd/csrc/error_plan.hpp"

using namespace ofdm;

static const char* const IDS[ERR_REFUSALS] = {
    "ok", "args", "device", "precision", "no_data", "pilots", "nfft", "stream", "modes", "sc_ref", "channel", "tap_delay",
    "tap_count", "fade_count", "fade_missing", "fade_delay", "fade_twice", "fade_power", "register", "descr_needed",
    "descr_unwanted", "points_missing", "points_many", "mmse_points", "mmse_fading", "chunk_cap", "mer_skip", "nmse_mp",
    "frames", "frame_bits", "receiver", "side", "task5_imp", "gap_bins", "output"};

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
  s.descr = (uint32_t)num(kv, "descr"); s.mmse = (int)num(kv, "mmse");
  s.device = (int)num(kv, "device"); s.ctx_device = (int)num(kv, "ctx_device");
  return s;
}

static ErrTablesWanted tables(const KV& kv) {
  ErrTablesWanted t;
  t.gap_bins = (int)num(kv, "gap_bins");
  t.out = num(kv, "out") != 0;
  return t;
}

static int answer(int id, const TxfWhy& w) {
  if (id < 0 || id >= ERR_REFUSALS) { std::fprintf(stderr, "bad id %d\n", id); return 3; }
  if (id != TXF_OK) std::printf("refused %s %s\n", IDS[id], w.text);
  else std::printf("ok\n");
  return 0;
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
    TxfWhy w;
    if (cmd == "profile") {
      if (const int rc = answer(err_profile_prelude(num(kv, "plan") ? &s : nullptr, num(kv, "bits") != 0, num(kv, "ref") != 0,
                                                    num(kv, "n_frames"), tables(kv), w), w))
        return rc;
    } else if (cmd == "study") {
      std::vector<uint8_t> reg;
      const std::string r = str(kv, "reg", "none");
      if (r != "none") for (char ch : r) reg.push_back((uint8_t)(ch - '0'));
      const std::string hs = str(kv, "h", "none"), ts = str(kv, "taps", "none");
      std::vector<double> h;                                       // complex double or float pairs, read in the flags' precision
      std::vector<float> hf;
      if (hs != "none" && hs != "bad")
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
      const bool fading = ts != "none";
      ErrStudyArgs a;
      a.receiver = (int)num(kv, "receiver"); a.side = (int)num(kv, "side"); a.both_channels = fading && hs != "none";
      a.time_desync = (int)num(kv, "time_desync"); a.freq_desync = (int)num(kv, "freq_desync"); a.mp_desync = (int)num(kv, "mp_desync");
      TxfCall c(a.receiver == 4 ? (fading ? "ber_sweep_task4_fading" : "ber_sweep_task4")
                                : (fading ? "ber_sweep_task5_fading" : "ber_sweep_task5"),
                num(kv, "frame0"), num(kv, "fpp"), r == "none" ? nullptr : reg.data());
      c.plan = num(kv, "plan") ? &s : nullptr;
      c.out = true;
      c.f64_flag = num(kv, "f64_flag") != 0;
      c.mp_desync = a.mp_desync;
      const bool points = num(kv, "points") != 0;
      c.with_points(points ? snr.data() : nullptr, points ? seeds.data() : nullptr, num(kv, "n_points"), num(kv, "max_chunk"));
      c.with_imp((int)num(kv, "sto_mode"), (int)num(kv, "cfo_mode"));
      const void* hp = hs == "none" ? nullptr : hs == "bad" ? nullptr : c.f64_flag ? (const void*)h.data() : (const void*)hf.data();
      const int h_len = hs == "none" ? 0 : hs == "bad" ? 3 : (int)(h.size() / 2);
      if (fading) c.with_fading(delay.data(), power.data(), (int)delay.size());
      else c.with_h(hp, h_len);
      TxfChannel ch;
      TxfGains g;
      if (const int rc = answer(err_study_prelude(c, a, tables(kv), ch, g, w), w)) return rc;
    } else if (cmd == "chunk") {
      const int receiver = (int)num(kv, "receiver");
      const TxfUse u = err_use(receiver, num(kv, "scr") != 0, (int)num(kv, "fade_taps"));
      std::printf("%lld %zu %zu\n", (long long)err_chunk(s, u, receiver, num(kv, "fpp"), num(kv, "cap")), txf_frame_bytes(s, u),
                  err_bit_bytes(s));
    } else if (cmd == "pass") {
      const ErrPass p = err_pass(s, (int)num(kv, "gap_bins"), num(kv, "frames"));
      std::printf("%d %d %zu %lld %lld %u\n", p.threads, p.symbols_in_lds, p.lds, (long long)p.flush_frames, (long long)p.launch_frames,
                  p.grid);
    } else if (cmd == "pos") {
      const ErrPos p = err_position(num(kv, "i"), (int)num(kv, "nd"), (int)num(kv, "bps"));
      std::printf("%lld %d %d\n", (long long)p.s, p.d, p.r);
    } else if (cmd == "walk") {
      const int nd = (int)num(kv, "nd"), bps = (int)num(kv, "bps");
      const uint32_t rc = err_recip(bps);
      const ErrPos p0 = err_position(num(kv, "i"), nd, bps);
      for (int delta = 0; delta <= 32; ++delta) {
        ErrPos p = p0;
        err_advance(p, delta, nd, bps, rc);
        std::printf("%lld %d %d ", (long long)p.s, p.d, p.r);
      }
      ErrPos p = p0;
      for (int delta = 0; delta <= 32; ++delta) {
        if (delta) err_advance(p, 1, nd, bps, rc);
        std::printf(delta < 32 ? "%lld %d %d " : "%lld %d %d\n", (long long)p.s, p.d, p.r);
      }
    } else if (cmd == "div") {
      const int bps = (int)num(kv, "bps");
      for (int n = 0; n < 64; ++n) std::printf(n < 63 ? "%d " : "%d\n", err_small_div(n, err_recip(bps)));
    } else {
      std::fprintf(stderr, "unknown command %s\n", cmd.c_str());
      return 2;
    }
  }
  return 0;
}
