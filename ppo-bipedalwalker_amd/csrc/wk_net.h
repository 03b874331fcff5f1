// wk_net.h -- the network description of the general kernels (wk_net.hip, NetworkKernels = 1).
//
// A NetSpec is built from the two DSL strings of the configuration.  The grammar and the
// output-size rule are ConsoleRenderer.ValidateNeuralNetwork's (ConsoleRenderer.cs:662-682:
// "Input" then one or more "|n|" (n without a leading zero) or "(ReLU|LeakyReLU|TanH)" tokens,
// then "Output"; the last dense layer outputs 1 (critic) or 4 (actor)); the layer list is
// PPOAgent.ParseLayers' (PPOAgent.cs:106-142): the first dense layer reads the 12 state values.
// Parameter layout: the .weights order -- critic dense layers, then the actor's, each W
// (out x in, row-major) then b -- so the default strings give wk_common.h's OFF_* and NPARAM.
//
// Host code only, no HIP: tests/cpp/net_spec_check.cpp builds it with a plain C++ compiler.
// NetDesc is plain data and goes to the kernels by value.
#ifndef WK_NET_H
#define WK_NET_H
#include <climits>
#include <cstdio>
#include <cstring>
#include <string>

namespace wk {

enum : int { NET_STATE = 12, NET_MAX_LAYERS = 8, NET_MAX_DENSE = 4, NET_MAX_WIDTH = 128 };
enum : int { NL_DENSE = 0, NL_RELU = 1, NL_LRELU = 2, NL_TANH = 3 };

struct NetLayer {
  int kind;      // NL_*
  int in, out;   // widths (activation: in == out)
  int off_w;     // dense: W at params[off_w] (out x in), b at params[off_b]
  int off_b;
  int dense;     // dense: index among the network's dense layers
  int row_in;    // first row of the layer's input in a wave's activation cache (wk_net.hip)
  int row_out;   // first row of its output
};

struct NetDesc {
  int n_layers, n_dense;
  int n_out;     // width of the network's output
  int row_end;   // first row of the output (== the last layer's row_out; 0 rows: the input)
  int rows;      // rows of the activation cache: every layer boundary, each padded to 4
  int off, n_params;  // this network's span of the flat parameter vector
  NetLayer layer[NET_MAX_LAYERS];
};

inline const char* net_default_critic() { return "Input |64| (LeakyReLU) |1| Output"; }
inline const char* net_default_actor() {
  return "Input |64| (LeakyReLU) |64| (LeakyReLU) |4| (TanH) Output";
}

// One token of the string: a dense width (kind NL_DENSE, value saturating at INT_MAX) or an
// activation.  Tokens of any number (the limits are net_build's).
struct NetToken { int kind, width; };

// The grammar alone: true and the token count, or false.  `visit` (may be null) sees each token.
template <class F>
inline bool net_scan(const char* s, F&& visit) {
  if (!s || strncmp(s, "Input ", 6) != 0) return false;
  const char* p = s + 6;
  int count = 0;
  for (;;) {
    if (*p == '|') {
      const char* q = p + 1;
      if (*q < '1' || *q > '9') return false;  // "|0|", leading zeros, "||"
      long long v = 0;
      while (*q >= '0' && *q <= '9') {
        if (v <= INT_MAX) v = v * 10 + (*q - '0');
        q++;
      }
      if (q[0] != '|' || q[1] != ' ') return false;
      visit(NetToken{NL_DENSE, v > INT_MAX ? INT_MAX : (int)v});
      p = q + 2;
    } else if (*p == '(') {
      int kind;
      size_t len;
      if (strncmp(p, "(LeakyReLU) ", 12) == 0) { kind = NL_LRELU; len = 12; }
      else if (strncmp(p, "(TanH) ", 7) == 0) { kind = NL_TANH; len = 7; }
      else if (strncmp(p, "(ReLU) ", 7) == 0) { kind = NL_RELU; len = 7; }
      else return false;
      visit(NetToken{kind, 0});
      p += len;
    } else {
      break;
    }
    count++;
  }
  return count > 0 && strcmp(p, "Output") == 0;
}

// ConsoleRenderer.ValidateNeuralNetwork (:661-682) with its two messages
inline bool valid_network(const char* s, bool critic, std::string& why) {
  int last = 0;  // (no dense layer at all: "currently outputs 0")
  if (!net_scan(s, [&](const NetToken& t) { if (t.kind == NL_DENSE) last = t.width; })) {
    why = "neural network not valid, check syntax";
    return false;
  }
  const int need = critic ? 1 : 4;
  if (last != need) {
    why = "last dense layer should output " + std::to_string(need) + ", currently outputs " +
          std::to_string(last);
    return false;
  }
  return true;
}

// The layer list of a valid string within the general kernels' limits; `off` is the network's
// first parameter.  False and a message naming the limit and the value otherwise.
inline bool net_build(const char* s, bool critic, int off, NetDesc& d, std::string& why) {
  const char* who = critic ? "critic" : "actor";
  if (!valid_network(s, critic, why)) {
    why = std::string(who) + " network '" + (s ? std::string(s).substr(0, 200) : std::string("(null)")) +
          "': " + why;
    return false;
  }
  memset(&d, 0, sizeof d);
  int total = 0, dense = 0, width_bad = 0;
  net_scan(s, [&](const NetToken& t) {
    total++;
    if (t.kind == NL_DENSE) {
      dense++;
      if (t.width > NET_MAX_WIDTH && !width_bad) width_bad = t.width;
    }
  });
  char b[160];
  if (width_bad) {
    snprintf(b, sizeof b, "%s network: layer width %d exceeds the general kernels' limit of %d", who,
             width_bad, (int)NET_MAX_WIDTH);
    why = b;
    return false;
  }
  if (total > NET_MAX_LAYERS) {
    snprintf(b, sizeof b, "%s network: %d layers exceed the general kernels' limit of %d layers "
             "(dense and activation together)", who, total, (int)NET_MAX_LAYERS);
    why = b;
    return false;
  }
  if (dense > NET_MAX_DENSE) {
    snprintf(b, sizeof b, "%s network: %d dense layers exceed the general kernels' limit of %d dense "
             "layers", who, dense, (int)NET_MAX_DENSE);
    why = b;
    return false;
  }
  int width = NET_STATE, row = 0, p = off, nd = 0, nl = 0;
  net_scan(s, [&](const NetToken& t) {
    NetLayer& L = d.layer[nl++];
    L.kind = t.kind;
    L.in = width;
    L.out = t.kind == NL_DENSE ? t.width : width;
    L.row_in = row;
    row += (width + 3) / 4 * 4;
    L.row_out = row;
    if (t.kind == NL_DENSE) {
      L.off_w = p;
      L.off_b = p + L.out * L.in;
      p = L.off_b + L.out;
      L.dense = nd++;
    }
    width = L.out;
  });
  d.n_layers = nl;
  d.n_dense = nd;
  d.n_out = width;
  d.row_end = row;
  d.rows = row + (width + 3) / 4 * 4;
  d.off = off;
  d.n_params = p - off;
  return true;
}

struct NetSpec {
  std::string critic_str, actor_str;
  NetDesc critic, actor;
  int np;  // critic.n_params + actor.n_params
};

// NULL: the default string
inline bool net_spec(const char* critic, const char* actor, NetSpec& s, std::string& why) {
  s.critic_str = critic ? critic : net_default_critic();
  s.actor_str = actor ? actor : net_default_actor();
  if (!net_build(s.critic_str.c_str(), true, 0, s.critic, why)) return false;
  if (!net_build(s.actor_str.c_str(), false, s.critic.n_params, s.actor, why)) return false;
  s.np = s.critic.n_params + s.actor.n_params;
  return true;
}

}  // namespace wk
#endif
