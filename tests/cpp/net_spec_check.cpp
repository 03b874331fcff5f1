// net_spec_check.cpp -- the network-string parser of the general kernels (csrc/wk_net.h) on the
// test networks and on hostile input: empty, truncated, very long, over every limit.  Host code
// only; tests/test_net_dsl.py builds it with -fsanitize=address,undefined and runs it.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "wk_net.h"

static int failures = 0;
#define CHECK(cond)                                                         \
  do {                                                                      \
    if (!(cond)) { printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); failures++; } \
  } while (0)

static bool spec(const std::string& c, const std::string& a, wk::NetSpec& s, std::string& why) {
  // exact-size heap copies: a read past the terminator is an AddressSanitizer report
  std::vector<char> cb(c.begin(), c.end()), ab(a.begin(), a.end());
  cb.push_back(0);
  ab.push_back(0);
  return wk::net_spec(cb.data(), ab.data(), s, why);
}

int main() {
  const std::string cd = wk::net_default_critic(), ad = wk::net_default_actor();
  wk::NetSpec s;
  std::string why;

  CHECK(wk::net_spec(nullptr, nullptr, s, why));
  CHECK(s.critic.n_params == 897 && s.actor.n_params == 5252 && s.np == 6149);
  CHECK(s.critic.n_layers == 3 && s.critic.n_dense == 2 && s.actor.n_layers == 6 && s.actor.n_dense == 3);
  CHECK(s.actor.off == 897 && s.actor.layer[0].off_w == 897 && s.actor.layer[0].off_b == 897 + 768);
  CHECK(s.actor.layer[2].off_w == 897 + 832 && s.actor.layer[4].off_b == 897 + 832 + 4096 + 64 + 256);

  CHECK(spec("Input |1| Output", "Input |4| Output", s, why));
  CHECK(s.critic.n_params == 13 && s.actor.n_params == 52 && s.critic.n_layers == 1);

  CHECK(spec("Input |5| (TanH) (ReLU) |1| Output",
             "Input (TanH) |7| (ReLU) |17| |33| (LeakyReLU) |4| Output", s, why));
  CHECK(s.critic.n_params == 5 * 12 + 5 + 5 + 1);
  CHECK(s.actor.n_params == 7 * 12 + 7 + 17 * 7 + 17 + 33 * 17 + 33 + 4 * 33 + 4);
  CHECK(s.actor.layer[0].kind == wk::NL_TANH && s.actor.layer[0].in == 12 && s.actor.layer[1].in == 12);
  CHECK(s.actor.n_layers == 7 && s.actor.n_dense == 4 && s.actor.n_out == 4);
  for (int l = 0; l < s.actor.n_layers; l++) {  // the cache rows: every boundary, padded to 4
    const wk::NetLayer& L = s.actor.layer[l];
    CHECK(L.row_out == L.row_in + (L.in + 3) / 4 * 4);
    CHECK(L.row_out + L.out <= s.actor.rows);
  }

  CHECK(spec("Input |128| (LeakyReLU) |128| (ReLU) |128| (TanH) |1| Output",
             "Input |128| (ReLU) |128| (TanH) |128| (LeakyReLU) |4| (TanH) Output", s, why));
  CHECK(s.np == 70021 && s.actor.n_layers == 8 && s.critic.n_layers == 7);
  CHECK(s.actor.rows <= wk::NET_STATE + wk::NET_MAX_LAYERS * wk::NET_MAX_WIDTH);

  // limits: the message names the limit and the value
  CHECK(!spec("Input |129| (ReLU) |1| Output", ad, s, why) && why.find("width 129") != std::string::npos);
  CHECK(!spec(cd, "Input |8| |8| |8| |8| |4| Output", s, why) && why.find("5 dense") != std::string::npos);
  CHECK(!spec(cd, "Input (ReLU) (ReLU) (ReLU) (ReLU) (ReLU) (ReLU) (ReLU) (ReLU) |4| Output", s, why) &&
        why.find("9 layers") != std::string::npos);
  CHECK(!spec("Input |99999999999999999999| |1| Output", ad, s, why) && why.find("width") != std::string::npos);
  // grammar and output sizes (ConsoleRenderer.ValidateNeuralNetwork)
  CHECK(!spec("Input |0| |1| Output", ad, s, why) && why.find("not valid") != std::string::npos);
  CHECK(!spec("Input |064| |1| Output", ad, s, why));
  CHECK(!spec(cd, "Input |64| |3| Output", s, why) && why.find("should output 4, currently outputs 3") != std::string::npos);
  CHECK(!spec(cd, "Input |64| (Sigmoid) |4| Output", s, why));
  CHECK(!spec("Input (ReLU) Output", ad, s, why) && why.find("currently outputs 0") != std::string::npos);
  CHECK(!spec("", ad, s, why) && !spec("Input", ad, s, why) && !spec("Input ", ad, s, why));
  CHECK(!spec("Input Output", ad, s, why) && !spec("Input  |1| Output", ad, s, why));
  CHECK(!spec("Input |1| Output ", ad, s, why) && !spec("input |1| Output", ad, s, why));
  CHECK(!spec("Input |1|Output", ad, s, why) && !spec("Input |-1| Output", ad, s, why));
  CHECK(!spec("Input |1 | Output", ad, s, why) && !spec("Input || Output", ad, s, why));
  // every truncation of a valid string is refused (and reads nothing past its end)
  for (size_t k = 0; k < ad.size(); k++) CHECK(!spec(cd, ad.substr(0, k), s, why));
  for (size_t k = 0; k < cd.size(); k++) CHECK(!spec(cd.substr(0, k), ad, s, why));
  // very long strings: grammatical ones trip the limits, the others the grammar
  std::string longv = "Input ";
  for (int i = 0; i < 200000; i++) longv += "(ReLU) ";
  CHECK(!spec(longv + "|1| Output", ad, s, why) && why.find("layers") != std::string::npos);
  CHECK(!spec(longv, ad, s, why) && !spec(longv + "|1|", ad, s, why));
  CHECK(!spec("Input |" + std::string(100000, '7') + "| |1| Output", ad, s, why));
  CHECK(!spec(std::string(1 << 20, '|'), ad, s, why));

  std::string msg;
  CHECK(wk::valid_network(cd.c_str(), true, msg) && !wk::valid_network(cd.c_str(), false, msg));
  CHECK(!wk::valid_network(nullptr, true, msg) && msg == "neural network not valid, check syntax");

  if (failures) return 1;
  printf("net_spec_check ok\n");
  return 0;
}
