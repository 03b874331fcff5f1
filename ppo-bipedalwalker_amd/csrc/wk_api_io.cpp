// wk_api_io.cpp -- what the context reads and writes: the weights text format, the binary
// checkpoint with its kinds and sections, and the in-memory snapshot.
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "wk_ctx.h"
#include "wk_text.h"

// (also the data file's writer, wk_api_rollout.cpp)
bool write_file(const char* path, const void* data, size_t n) {
  FILE* f = fopen(path, "wb");
  if (!f) return false;
  const bool ok = fwrite(data, 1, n, f) == n;
  return fclose(f) == 0 && ok;
}

// ---------------- weights text format + binary checkpoint ----------
// Reference format (PPOAgent.Save PPOAgent.cs:192-213 -> NeuralNetwork.Save
// NeuralNetwork.cs:159-176 -> DenseLayer.Save DenseLayer.cs:73-79 -> Matrix.Save
// Matrix.cs:133-153): one file per network, line 0 the network DSL string, then one line
// per dense layer "W w00 w01 ... B b0 b1 ..." (row-major out x in, values joined by one
// space).  Values are written as .NET Core 3.0+'s float.ToString() writes them under
// en-US: shortest round-trip digits, "E-05" / "E+09"-style exponents for |v| < 1e-4 or
// >= 1e9, "-0", "NaN", "∞".  Parsing accepts strtof syntax plus "∞" (a superset of the
// digit strings float.Parse reads; "Infinity" and "NaN" included).

namespace {
struct DenseSpec { int off_w, rows, cols, off_b; };
// the dense layers of a network description, in order
std::vector<DenseSpec> dense_layers(const wk::NetDesc& d) {
  std::vector<DenseSpec> v;
  for (int l = 0; l < d.n_layers; l++)
    if (d.layer[l].kind == wk::NL_DENSE)
      v.push_back({d.layer[l].off_w, d.layer[l].out, d.layer[l].in, d.layer[l].off_b});
  return v;
}
std::string format_network(const float* p, const char* dsl, const wk::NetDesc& net) {
  const std::vector<DenseSpec> layers = dense_layers(net);
  const int nl = (int)layers.size();
  std::string text = std::string(dsl) + "\n";
  for (int l = 0; l < nl; l++) {
    const DenseSpec& d = layers[l];
    std::string line = "W";
    for (int i = 0; i < d.rows * d.cols; i++) line += " " + wk::dotnet_float(p[d.off_w + i]);
    line += " B";
    for (int i = 0; i < d.rows; i++) line += " " + wk::dotnet_float(p[d.off_b + i]);
    text += line + "\n";
  }
  return text;
}

// NeuralNetwork.Load / ValidateWeights / DenseLayer.Load semantics: the DSL line must
// match, every token must parse, and each layer needs rows*cols weights then rows biases.
int parse_network(const char* text, const char* dsl, const wk::NetDesc& net, float* p,
                  std::string& why) {
  const std::vector<DenseSpec> layers = dense_layers(net);
  const int nl = (int)layers.size();
  std::vector<std::string> lines;
  std::string cur;
  for (const char* q = text; *q; q++) {
    if (*q == '\n') { lines.push_back(cur); cur.clear(); }
    else if (*q != '\r') cur += *q;
  }
  if (!cur.empty()) lines.push_back(cur);
  if ((int)lines.size() < nl + 1) { why = "weights file too short"; return WK_ERR_ARG; }
  if (lines[0] != dsl) { why = "network string '" + lines[0] + "' does not match '" + dsl + "'"; return WK_ERR_CONFIG; }
  for (int l = 0; l < nl; l++) {
    const DenseSpec& d = layers[l];
    const std::string& s = lines[l + 1];
    const size_t w = s.find('W'), b = s.find('B');
    if (w == std::string::npos || b == std::string::npos || b < w) { why = "weights structure issue"; return WK_ERR_ARG; }
    // "W a b c B d e": tokens separated by single spaces (ValidateWeights splits with
    // string.Split(), so an empty token fails float.TryParse)
    auto parse_list = [&](const std::string& seg, float* dst, int count) -> bool {
      if (seg.size() < 2 || seg.front() != ' ') return false;
      size_t at = 1;
      for (int i = 0; i < count; i++) {
        const size_t sp = seg.find(' ', at);
        const std::string tok = seg.substr(at, sp == std::string::npos ? std::string::npos : sp - at);
        if (tok.empty()) return false;
        if (tok == "\xe2\x88\x9e") dst[i] = INFINITY;
        else if (tok == "-\xe2\x88\x9e") dst[i] = -INFINITY;
        else {
          char* end = nullptr;
          dst[i] = strtof(tok.c_str(), &end);
          if (*end) return false;
        }
        if (sp == std::string::npos) return i == count - 1;
        at = sp + 1;
      }
      return at == seg.size();  // the weights segment ends with the space before "B"
    };
    if (!parse_list(s.substr(w + 1, b - w - 1), p + d.off_w, d.rows * d.cols)) { why = "error in weights section"; return WK_ERR_ARG; }
    if (!parse_list(s.substr(b + 1), p + d.off_b, d.rows)) { why = "error in biases section"; return WK_ERR_ARG; }
  }
  return WK_OK;
}

bool read_file(const char* path, std::string& out) {
  FILE* f = fopen(path, "rb");
  if (!f) return false;
  char buf[65536];
  size_t k;
  while ((k = fread(buf, 1, sizeof buf, f)) > 0) out.append(buf, k);
  fclose(f);
  return true;
}

const uint32_t kCkptMagic = 0x4B434B57u;  // "WKCK"
struct CkptHeader {
  uint32_t magic, version, n_env, nstate, nparam, adam_t;
  uint64_t seed;
  int32_t env_offset, iterations, max_timesteps;
  uint32_t rollout_steps;
};
static_assert(sizeof(CkptHeader) == 48, "checkpoint header");
// version 4 adds this block right after the header: the configuration that changes the
// physics beyond the header's fields (RoughFloor) and the mapping the file was written with
struct CkptExt {
  int32_t rough_floor, lanes_per_walker, general, learn;  // (the last two: 1 or 0, see CkptKind)
};
static_assert(sizeof(CkptExt) == 16, "checkpoint extension");
// 3: + scene section (int32 n_props, wk_prop[n_props], [n][pstride]); 4: + CkptExt
const uint32_t kCkptVersion = 4;
// 5: a general-network context (NetworkKernels = 1; CkptExt.general = 1): after CkptExt two
// uint32 lengths and the critic and actor strings, and nparam parameters of that network.  A
// built-in context still writes version 4, byte for byte as before
const uint32_t kCkptVersionNet = 5;
// 6: a LearnLogStd = 1 context of either kernel family (CkptExt.learn = 1; general still
// tells the family): after the version-5 network section, if any, the trained log-std and its
// Adam state.  A LearnLogStd = 0 context still writes version 4 or 5, byte for byte as before
const uint32_t kCkptVersionLogStd = 6;
#pragma pack(push, 4)
struct CkptLogStd {
  float log_std;
  int32_t t;
  double m, v;
};
#pragma pack(pop)
static_assert(sizeof(CkptLogStd) == 24, "checkpoint log-std section");
// 7: a context with reward normalisation enabled, of either kernel family, with or without a
// trained log-std (CkptExt.general / learn tell which, as in version 6): after the scene
// section, at the end of the file, this record and acc[n_env].  A context not enabled still
// writes version 4, 5 or 6, byte for byte as before
const uint32_t kCkptVersionRnorm = 7;
struct CkptRnorm {
  int32_t enable, frozen;
  float clip, epsilon;
  int64_t count;
  double mean, m2;
  float scale;
  int32_t pad;
};
static_assert(sizeof(CkptRnorm) == 48, "checkpoint reward-normalisation section");
// What a checkpoint holds beyond version 4's sections.  The three flags decide the version a
// context writes and CkptExt's two flags, and so what a file denotes: the one place that knows
struct CkptKind { bool general, learn, rnorm; };
CkptKind ckpt_kind(const wk_ctx* c) { return {c->general, c->cfg.LearnLogStd == 1, c->rn_on != 0}; }
uint32_t ckpt_version(const CkptKind& k) {
  return k.rnorm ? kCkptVersionRnorm : k.learn ? kCkptVersionLogStd : k.general ? kCkptVersionNet : kCkptVersion;
}
// The kind f a file's (version, CkptExt) pair denotes: versions 4 and 5 say it themselves, 6 leaves
// the kernel family to CkptExt, 7 both flags.  WK_OK where that is the context's own kind;
// WK_ERR_ARG with the refusal's text where it is another or CkptExt contradicts the version
int ckpt_file_kind(wk_ctx* c, const char* path, uint32_t version, const CkptExt& ext) {
  const CkptKind mine = ckpt_kind(c);
  CkptKind f{};
  f.rnorm = version >= kCkptVersionRnorm;
  if (f.rnorm != mine.rnorm) {
    if (f.rnorm)
      SETERR(c, "checkpoint '%s' is version %u, written with reward normalisation enabled: enable it on "
                "this context first (wk_reward_norm_config)", path, version);
    else
      SETERR(c, "checkpoint '%s' is version %u: a context with reward normalisation enabled loads only "
                "version %u files", path, version, kCkptVersionRnorm);
    return WK_ERR_ARG;
  }
  // the networks first: a file of other networks (or of the other kind of kernels) has another
  // parameter count and layout
  f.learn = f.rnorm ? ext.learn != 0 : version >= kCkptVersionLogStd;
  f.general = f.learn || f.rnorm ? ext.general != 0 : version >= kCkptVersionNet;
  if (f.learn != mine.learn || (ext.learn != 0) != f.learn) {
    SETERR(c, "checkpoint '%s' was written with LearnLogStd %d (context: %d)", path, f.learn ? 1 : 0,
           c->cfg.LearnLogStd);
    return WK_ERR_ARG;
  }
  if (f.general != mine.general || (ext.general != 0) != mine.general) {
    SETERR(c, "checkpoint '%s' was written with NetworkKernels %d (context: %d)", path,
           f.general ? 1 : 0, mine.general ? 1 : 0);
    return WK_ERR_ARG;
  }
  return WK_OK;
}
// The file's fixed sections, in file order, between its variable head (header, CkptExt, the
// version-5 network section) and its scene section: the only place that knows the order
std::array<Seg, 9> ckpt_sections(const wk_ctx* c) {
  const size_t n = c->n, wbytes = sizeof(float) * c->np;
  return {{{c->W, wbytes}, {c->m, wbytes}, {c->v, wbytes}, {c->st, sizeof(float) * wk::NSTATE * n},
           {c->rng_t, sizeof(uint32_t) * n}, {c->dxoff, sizeof(float) * n}, {c->mat, sizeof(int32_t) * n},
           {c->ep_acc, sizeof(double) * n}, {c->ep_len, sizeof(int32_t) * n}}};
}
// the bytes of the sections before the one held in `until` (null: of all of them)
size_t ckpt_offset(const wk_ctx* c, const void* until) {
  size_t off = 0;
  for (const Seg& g : ckpt_sections(c)) {
    if (g.p == until) break;
    off += g.bytes;
  }
  return off;
}
}  // namespace

int wk_format_weights(const float* params, char* critic, size_t critic_cap, char* actor,
                      size_t actor_cap) {
  return wk_format_weights_net(nullptr, nullptr, params, critic, critic_cap, actor, actor_cap);
}

int wk_parse_weights(const char* critic, const char* actor, float* params) {
  return wk_parse_weights_net(nullptr, nullptr, critic, actor, params);
}

int wk_net_param_count(const char* critic, const char* actor, int* n_critic, int* n_actor) {
  wk::NetSpec ns;
  std::string why;
  if (!wk::net_spec(critic, actor, ns, why)) { wk::set_last_error(why); return WK_ERR_CONFIG; }
  if (n_critic) *n_critic = ns.critic.n_params;
  if (n_actor) *n_actor = ns.actor.n_params;
  return WK_OK;
}

int wk_num_params(wk_ctx* c, int* n_critic, int* n_actor) {
  if (!c) return WK_ERR_ARG;
  if (n_critic) *n_critic = c->net.critic.n_params;
  if (n_actor) *n_actor = c->net.actor.n_params;
  return WK_OK;
}

int wk_format_weights_net(const char* critic_net, const char* actor_net, const float* params,
                          char* critic, size_t critic_cap, char* actor, size_t actor_cap) {
  if (!params) return WK_ERR_ARG;
  wk::NetSpec ns;
  std::string why;
  if (!wk::net_spec(critic_net, actor_net, ns, why)) { wk::set_last_error(why); return WK_ERR_CONFIG; }
  const std::string c = format_network(params, ns.critic_str.c_str(), ns.critic);
  const std::string a = format_network(params, ns.actor_str.c_str(), ns.actor);
  if (!critic || !actor || critic_cap < c.size() + 1 || actor_cap < a.size() + 1)
    return -(int)(c.size() > a.size() ? c.size() + 1 : a.size() + 1);  // needed capacity
  memcpy(critic, c.c_str(), c.size() + 1);
  memcpy(actor, a.c_str(), a.size() + 1);
  return WK_OK;
}

int wk_parse_weights_net(const char* critic_net, const char* actor_net, const char* critic,
                         const char* actor, float* params) {
  if (!critic || !actor || !params) { wk::set_last_error("null argument"); return WK_ERR_ARG; }
  wk::NetSpec ns;
  std::string why;
  if (!wk::net_spec(critic_net, actor_net, ns, why)) { wk::set_last_error(why); return WK_ERR_CONFIG; }
  std::vector<float> p(ns.np, 0.0f);
  int r = parse_network(critic, ns.critic_str.c_str(), ns.critic, p.data(), why);
  if (r == WK_OK) r = parse_network(actor, ns.actor_str.c_str(), ns.actor, p.data(), why);
  if (r != WK_OK) { wk::set_last_error(why); return r; }
  memcpy(params, p.data(), sizeof(float) * ns.np);
  return WK_OK;
}

int wk_save_weights(wk_ctx* c, const char* critic_path, const char* actor_path) {
  DevGuard dg_(c);
  if (!c || !critic_path || !actor_path) return WK_ERR_ARG;
  std::vector<float> p(c->np);
  int r = wk_get_weights(c, p.data());
  if (r) return r;
  const std::string ct = format_network(p.data(), c->net.critic_str.c_str(), c->net.critic);
  const std::string at = format_network(p.data(), c->net.actor_str.c_str(), c->net.actor);
  if (!write_file(critic_path, ct.data(), ct.size()) || !write_file(actor_path, at.data(), at.size())) {
    SETERR(c, "cannot write weights files '%s' / '%s'", critic_path, actor_path);
    return WK_ERR_ARG;
  }
  return WK_OK;
}

int wk_load_weights(wk_ctx* c, const char* critic_path, const char* actor_path) {
  DevGuard dg_(c);
  if (!c || !critic_path || !actor_path) return WK_ERR_ARG;
  std::string ct, at;
  if (!read_file(critic_path, ct) || !read_file(actor_path, at)) {
    SETERR(c, "cannot read weights files '%s' / '%s'", critic_path, actor_path);
    return WK_ERR_ARG;
  }
  std::vector<float> p(c->np, 0.0f);
  std::string why;
  int r = parse_network(ct.c_str(), c->net.critic_str.c_str(), c->net.critic, p.data(), why);
  if (r == WK_OK) r = parse_network(at.c_str(), c->net.actor_str.c_str(), c->net.actor, p.data(), why);
  if (r != WK_OK) { c->err = why; return r; }
  return wk_set_weights(c, p.data());
}

// a version-5 file's network section: two uint32 lengths, then the critic and actor strings
static std::string net_section(const wk_ctx* c) {
  const uint32_t len[2] = {(uint32_t)c->net.critic_str.size(), (uint32_t)c->net.actor_str.size()};
  return std::string((const char*)len, sizeof len) + c->net.critic_str + c->net.actor_str;
}

// Binary checkpoint for exact resume: weights, Adam m / v / t, every walker record,
// Philox step counters, start offsets and materials.
int wk_checkpoint_save(wk_ctx* c, const char* path) {
  DevGuard dg_(c);
  if (!c || !path) return WK_ERR_ARG;
  const size_t n = c->n;
  const CkptKind k = ckpt_kind(c);
  CkptHeader h{kCkptMagic, ckpt_version(k), (uint32_t)n, (uint32_t)wk::NSTATE,
               (uint32_t)c->np, (uint32_t)c->adam_t, c->seed, c->cfg.EnvOffset, c->cfg.Iterations,
               c->cfg.MaxTimesteps, c->rollout_steps};
  const int np = c->scene.n_props;
  const size_t scene_bytes = sizeof(int32_t) + sizeof(wk_prop) * np + sizeof(float) * n * c->scene.pstride;
  const CkptExt ext{c->cfg.RoughFloor, c->P.lanes, k.general ? 1 : 0, k.learn ? 1 : 0};
  std::string nets = k.general ? net_section(c) : std::string();
  if (k.learn) {  // (the variable head: network section, then the log-std section)
    const CkptLogStd ls{c->P.log_std, c->ls.t, c->ls.m, c->ls.v};
    nets.append((const char*)&ls, sizeof ls);
  }
  const size_t rnorm_bytes = k.rnorm ? sizeof(CkptRnorm) + sizeof(float) * n : 0;
  std::vector<char> buf(sizeof h + sizeof ext + nets.size() + ckpt_offset(c, nullptr) + scene_bytes + rnorm_bytes);
  char* q = buf.data();
  memcpy(q, &h, sizeof h); q += sizeof h;
  memcpy(q, &ext, sizeof ext); q += sizeof ext;
  memcpy(q, nets.data(), nets.size()); q += nets.size();
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (const Seg& g : ckpt_sections(c)) {
    HIPCHK(c, hipMemcpy(q, g.p, g.bytes, hipMemcpyDeviceToHost));
    q += g.bytes;
  }
  const int32_t np32 = np;
  memcpy(q, &np32, sizeof np32); q += sizeof np32;
  if (np > 0) {
    memcpy(q, c->scene_desc.data(), sizeof(wk_prop) * np); q += sizeof(wk_prop) * np;
    HIPCHK(c, hipMemcpy(q, c->props, sizeof(float) * n * c->scene.pstride, hipMemcpyDeviceToHost));
    q += sizeof(float) * n * c->scene.pstride;
  }
  if (k.rnorm) {
    wk::RnormRec r;
    HIPCHK(c, hipMemcpy(&r, c->rn_rec, sizeof r, hipMemcpyDeviceToHost));
    const CkptRnorm s{c->rn_on, c->rn_frozen, c->rn_clip, c->rn_eps, r.count, r.mean, r.m2, r.scale, 0};
    memcpy(q, &s, sizeof s); q += sizeof s;
    HIPCHK(c, hipMemcpy(q, c->rn_acc, sizeof(float) * n, hipMemcpyDeviceToHost));
  }
  if (!write_file(path, buf.data(), buf.size())) { SETERR(c, "cannot write checkpoint '%s'", path); return WK_ERR_ARG; }
  return WK_OK;
}

// Every check runs before the first device write, so a rejected file leaves the context
// exactly as it was: header, sizes, seed / EnvOffset (the Philox streams),
// Iterations / MaxTimesteps / RoughFloor (the physics), and the scene's acceptability.
int wk_checkpoint_load(wk_ctx* c, const char* path) {
  DevGuard dg_(c);
  if (!c || !path) return WK_ERR_ARG;
  std::string data;
  if (!read_file(path, data)) { SETERR(c, "cannot read checkpoint '%s'", path); return WK_ERR_ARG; }
  const size_t n = c->n;
  CkptHeader h;
  if (data.size() < sizeof h) { SETERR(c, "checkpoint '%s' truncated", path); return WK_ERR_ARG; }
  memcpy(&h, data.data(), sizeof h);
  if (h.magic != kCkptMagic || h.version < 2 || h.version > kCkptVersionRnorm) {
    SETERR(c, "'%s' is not a wk checkpoint", path);
    return WK_ERR_ARG;
  }
  // version 2 (before scene props) has no scene section, version 3 no CkptExt.  Neither
  // records RoughFloor (which already existed when they were written), and nothing in the
  // walker records tells the floors apart: loading one could run the wrong physics on the
  // saved walkers, so it is refused
  if (h.version < 4) {
    SETERR(c, "checkpoint '%s' is version %u: its floor type (RoughFloor) was not recorded "
              "before version 4, so it cannot be resumed safely", path, h.version);
    return WK_ERR_CONFIG;
  }
  size_t ext_bytes = sizeof(CkptExt);
  CkptExt ext{0, 0, 0, 0};
  if (data.size() >= sizeof h + ext_bytes) memcpy(&ext, data.data() + sizeof h, sizeof ext);
  if (int r = ckpt_file_kind(c, path, h.version, ext)) return r;
  const CkptKind file = ckpt_kind(c);  // (the file's is the context's from here on)
  if (file.general) {
    const std::string mine = net_section(c);
    if (data.size() < sizeof h + ext_bytes + mine.size() ||
        memcmp(data.data() + sizeof h + ext_bytes, mine.data(), mine.size()) != 0) {
      SETERR(c, "checkpoint '%s' was written for other networks than this context's '%s' / '%s'", path,
             c->net.critic_str.c_str(), c->net.actor_str.c_str());
      return WK_ERR_ARG;
    }
    ext_bytes += mine.size();
  }
  CkptLogStd ls{};
  if (file.learn) {  // its value is checked like wk_set_log_std's and wk_set_log_std_adam's
    if (data.size() < sizeof h + ext_bytes + sizeof ls) { SETERR(c, "checkpoint '%s' truncated", path); return WK_ERR_ARG; }
    memcpy(&ls, data.data() + sizeof h + ext_bytes, sizeof ls);
    if (!std::isfinite(ls.log_std) || ls.log_std < c->cfg.LogStdMin || ls.log_std > c->cfg.LogStdMax ||
        !std::isfinite(ls.m) || !std::isfinite(ls.v) || ls.v < 0.0 || ls.t < 0) {
      SETERR(c, "checkpoint '%s': invalid log-std section (log_std %g outside [%g, %g], or its Adam state)",
             path, (double)ls.log_std, (double)c->cfg.LogStdMin, (double)c->cfg.LogStdMax);
      return WK_ERR_ARG;
    }
    ext_bytes += sizeof ls;
  }
  size_t need = sizeof h + ext_bytes + ckpt_offset(c, nullptr) + sizeof(int32_t);
  int32_t np = 0;
  std::vector<wk_prop> desc;
  if (data.size() >= need) {
    memcpy(&np, data.data() + need - sizeof(int32_t), sizeof np);
    if (np < 0 || np > WK_MAX_PROPS) { SETERR(c, "checkpoint '%s': invalid scene section", path); return WK_ERR_ARG; }
    if (np > 0 && data.size() >= need + sizeof(wk_prop) * np) {
      desc.resize(np);
      memcpy(desc.data(), data.data() + need, sizeof(wk_prop) * np);
      need += sizeof(wk_prop) * np;
      size_t pstride = 0;
      for (const wk_prop& p : desc) {
        float xs[WK_PROP_MAXV], ys[WK_PROP_MAXV];
        const int nv = p.smooth >= 0 ? prop_vertices(p, p.smooth, xs, ys) : -1;
        pstride += nv > 0 ? (size_t)(2 * nv + 6) : (size_t)1 << 40;  // a bad record fails the size check
      }
      need += sizeof(float) * n * pstride;
    }
  }
  const size_t rnorm_bytes = file.rnorm ? sizeof(CkptRnorm) + sizeof(float) * n : 0;
  if (h.n_env != n || h.nstate != (uint32_t)wk::NSTATE || h.nparam != (uint32_t)c->np ||
      data.size() != need + rnorm_bytes) {
    SETERR(c, "checkpoint '%s' is for %u walkers (context has %zu)", path, h.n_env, n);
    return WK_ERR_ARG;
  }
  if (h.seed != c->seed || h.env_offset != c->cfg.EnvOffset) {  // the Philox streams differ
    SETERR(c, "checkpoint '%s' was written with seed %llu / EnvOffset %d (context: %llu / %d)",
           path, (unsigned long long)h.seed, h.env_offset, (unsigned long long)c->seed, c->cfg.EnvOffset);
    return WK_ERR_CONFIG;
  }
  if (h.iterations != c->cfg.Iterations || h.max_timesteps != c->cfg.MaxTimesteps ||
      ext.rough_floor != c->cfg.RoughFloor) {
    SETERR(c, "checkpoint '%s' was written with Iterations %d / MaxTimesteps %d / RoughFloor %d "
              "(context: %d / %d / %d)", path, h.iterations, h.max_timesteps, ext.rough_floor,
           c->cfg.Iterations, c->cfg.MaxTimesteps, c->cfg.RoughFloor);
    return WK_ERR_CONFIG;
  }
  CkptRnorm rn{};
  if (file.rnorm) {  // checked like wk_reward_norm_config's and wk_reward_norm_set's arguments
    memcpy(&rn, data.data() + need, sizeof rn);
    if (rn.enable != 1 || rn.frozen < 0 || rn.frozen > 1 || !(rn.clip > 0.0f) || !std::isfinite(rn.epsilon) ||
        rn.epsilon < 0.0f || rn.count < 0 || !std::isfinite(rn.mean) || !std::isfinite(rn.m2) || rn.m2 < 0.0 ||
        !std::isfinite(rn.scale) || !(rn.scale > 0.0f)) {
      SETERR(c, "checkpoint '%s': invalid reward-normalisation section", path);
      return WK_ERR_ARG;
    }
  }
  if (np > 0 && c->cfg.LanesPerWalker > 1) {  // wk_set_scene would refuse it
    SETERR(c, "checkpoint '%s' has scene props, which need the one-lane mapping "
              "(LanesPerWalker 0 or 1)", path);
    return WK_ERR_CONFIG;
  }
  {  // the walker records keep rigid template poles, checked before any write
    std::vector<float> rec(n * wk::NSTATE);
    memcpy(rec.data(), data.data() + sizeof h + ext_bytes + ckpt_offset(c, c->st),
           sizeof(float) * rec.size());
    if (int r = check_state_or_fail(c, rec.data())) return r;
  }
  // the scene first: wk_set_scene is all-or-nothing and is the last step that can fail on
  // anything but a device error
  if (int r = wk_set_scene(c, desc.data(), (int)desc.size()); r != WK_OK) return r;
  const char* q = data.data() + sizeof h + ext_bytes;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (const Seg& g : ckpt_sections(c)) {
    HIPCHK(c, hipMemcpy(g.p, q, g.bytes, hipMemcpyHostToDevice));
    if (g.p == c->dxoff) {  // the offsets also set the rough floor's lane order
      std::vector<float> dxh(n);
      std::memcpy(dxh.data(), q, sizeof(float) * n);
      HIPCHK(c, rough_order_upload(c, dxh.data()));
    }
    q += g.bytes;
  }
  if (np > 0) {
    q += sizeof(int32_t) + sizeof(wk_prop) * np;
    HIPCHK(c, hipMemcpy(c->props, q, sizeof(float) * n * c->scene.pstride, hipMemcpyHostToDevice));
  }
  c->adam_t = (int)h.adam_t;
  if (file.learn) {
    apply_log_std(c, ls.log_std);
    c->ls.m = ls.m; c->ls.v = ls.v; c->ls.t = ls.t;
  }
  if (file.rnorm) {  // the arguments, the statistics with their scale, the walkers' running returns
    wk::RnormRec r{};
    r.count = rn.count; r.mean = rn.mean; r.m2 = rn.m2;
    r.var = rn.count > 0 ? rn.m2 / (double)rn.count : 0.0;
    r.scale = rn.scale;
    HIPCHK(c, hipMemcpy(c->rn_rec, &r, sizeof r, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->rn_acc, data.data() + need + sizeof rn, sizeof(float) * n, hipMemcpyHostToDevice));
    c->rn_frozen = rn.frozen; c->rn_clip = rn.clip; c->rn_eps = rn.epsilon;
  }
  c->rollout_steps = h.rollout_steps;
  c->T_valid = 0;
  c->returns_valid = 0;
  c->vlast_valid = false;
  HIPCHK(c, upload_image(c));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return WK_OK;
}

// wk_snapshot's copy: the segments into the block at `base` one after the other, each from a
// multiple of 256 bytes on (op 0), or back out of it (op 1)
static int snap_copy(wk_ctx* c, int op, std::initializer_list<Seg> segs, void* base) {
  char* q = (char*)base;
  for (const Seg& g : segs) {
    if (g.bytes)
      HIPCHK(c, hipMemcpyAsync(op == 0 ? (void*)q : g.p, op == 0 ? g.p : (const void*)q, g.bytes,
                               hipMemcpyDeviceToDevice, c->stream));
    q += (g.bytes + 255) & ~(size_t)255;
  }
  return WK_OK;
}

int wk_snapshot(wk_ctx* c, int op) {
  DevGuard dg_(c);
  if (!c || op < 0 || op > 1) return WK_ERR_ARG;
  const size_t n = c->n;
  const std::initializer_list<Seg> segs = {
      {c->st, sizeof(float) * wk::NSTATE * n}, {c->rng_t, sizeof(uint32_t) * n},
      {c->W, sizeof(float) * c->np}, {c->Wz, c->Wz ? sizeof(float) * wk::mfma_image_floats() : 0},
      {c->m, sizeof(float) * c->np}, {c->v, sizeof(float) * c->np},
      {c->ep_acc, sizeof(double) * n}, {c->ep_len, sizeof(int32_t) * n},
      {c->ep_count, sizeof(uint64_t)},
      {c->props, c->props ? sizeof(float) * n * c->scene.pstride : 0}};
  size_t total = 0;
  for (const Seg& g : segs) total += (g.bytes + 255) & ~(size_t)255;
  if (op == 0) {
    if (ensure(c, &c->snap, &c->snap_bytes, total)) return WK_ERR_HIP;
    c->snap_host = {c->adam_t, c->P.log_std, c->ls, c->rollout_steps, c->loss_count};
    c->snap_log_drained = false;
  } else if (!c->snap_valid || c->snap_bytes < total) {
    SETERR(c, "no snapshot of this configuration to restore");
    return WK_ERR_STATE;
  }
  if (int r = snap_copy(c, op, segs, c->snap)) return r;
  // reward normalisation, on an enabled context: the walkers' running returns, then the record
  // (statistics and scale); a snapshot taken before the first enable holds none and restores none
  if (c->rn_on && (op == 0 || c->rn_snap_valid)) {
    const size_t acc_bytes = (sizeof(float) * n + 255) & ~(size_t)255;
    if (!c->rn_snap) HIPCHK(c, dev_alloc(c, &c->rn_snap, acc_bytes + sizeof(wk::RnormRec)));
    if (int r = snap_copy(c, op, {{c->rn_acc, sizeof(float) * n}, {c->rn_rec, sizeof(wk::RnormRec)}}, c->rn_snap))
      return r;
    if (op == 0) c->rn_snap_valid = true;
  } else if (op == 0) {
    c->rn_snap_valid = false;
  }
  if (op == 0) {
    c->snap_valid = true;
  } else {
    const wk_ctx::SnapHost& h = c->snap_host;
    c->adam_t = h.adam_t;
    // the trained log-std and its Adam state are part of the model; on a LearnLogStd = 0 context
    // the log-std is configuration (wk_set_log_std), like the learning rate, and stays
    if (c->cfg.LearnLogStd == 1) {
      apply_log_std(c, h.log_std);
      c->ls = h.ls;
    }
    c->rollout_steps = h.rollout_steps;
    c->loss_count = h.loss_count;
    // the records the saved count stood for were handed out by a drain since, and rollouts have
    // reused their slots: the log restarts empty (the running sums and lengths above are restored)
    if (c->snap_log_drained) HIPCHK(c, hipMemsetAsync(c->ep_count, 0, sizeof(uint64_t), c->stream));
    // the trajectory buffer is not part of the snapshot: it keeps the last rollout (the
    // counting replay reads its actions after a restore)
  }
  return WK_OK;
}
