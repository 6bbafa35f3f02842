// head_group.hip -- several independent trainers stepped in one launch sequence (include/acez.h, acez_train_group_*).
// Included by head_api.hip (it drives the trainers' own step phases). A group step advances every member by exactly one
// acez_train_step / acez_train_step_next: each member's gather, loss, weight-gradient / optimiser and schedule launches are the ones
// its own step issues, and the two dependent GEMM chains of all members run as ONE launch each (rowseq_group_kernel), whose bodies are
// rowseq_kernel's (rowgemm80_body<..., SEQ>): bitwise the members' own steps, in any order mixed with their single steps.
//
// Why: a workgroup of rowseq_kernel spends most of a layer filling its ring and waiting at the seam for its three siblings (~1.1 us of
// MFMA work in a 5.2-5.8 us layer). In the group chain a workgroup runs layer l of head 0, 1, ..., H-1 before layer l + 1 of head 0: the
// seam it waits on was closed while it worked on the other heads' tiles, and the next body's first W stages are requested behind the
// current epilogue exactly as between two layers of one head. Measured: 0.96 x the members' own steps at H = 3 --
// the members' activations together no longer fit the Infinity Cache -- so the session does not use it by default.
// The kernel is in the chain unit (head_kernels.hip), its argument structs in head_kernels.h; this is the host's half.

struct acez_train_group {
  std::vector<acez_trainer*> m;
  std::vector<const uint16_t*> in0;   // the buffer GroupHead::fwd[0] was built on (R[0] at creation)
  GroupHead* d_heads = nullptr;
  int n_fwd = 0, n_bwd = 0;
};

extern "C" void acez_train_group_destroy(acez_train_group* g) {
  if (!g) return;
  if (g->d_heads) (void)hipFree(g->d_heads);
  delete g;
}

extern "C" int acez_train_group_create(acez_train_group** out, acez_trainer* const* members, int h) {
  ACEZ_REQUIRE(out && members, "null pointer");
  ACEZ_REQUIRE(h >= 1 && h <= GROUP_MAX, "a group has 1 to 8 members");
  for (int i = 0; i < h; ++i) {
    const acez_trainer* t = members[i];
    ACEZ_REQUIRE(t, "null member");
    ACEZ_REQUIRE(!t->inference_only, "an inference-only context cannot be a group member");
    ACEZ_REQUIRE(t->cfg.pose_refinement == 0, "group members train without pose refinement");
    ACEZ_REQUIRE(t->cfg.refine_calibration == 0, "group members train without calibration refinement");
    for (int j = 0; j < i; ++j) ACEZ_REQUIRE(members[j] != t, "the same trainer is listed twice");
    const acez_trainer* t0 = members[0];
    ACEZ_REQUIRE(t->device == t0->device, "group members must be on one device");
    ACEZ_REQUIRE(t->f16 == t0->f16, "group members must have the same compute_dtype");
    ACEZ_REQUIRE(t->nb == t0->nb, "group members must have the same num_head_blocks");
    ACEZ_REQUIRE(t->cfg.head.use_homogeneous == t0->cfg.head.use_homogeneous, "group members must have the same use_homogeneous");
  }
  ACEZ_HIP_CHECK(hipSetDevice(members[0]->device));
  acez_train_group* g = new (std::nothrow) acez_train_group();
  ACEZ_REQUIRE(g, "out of host memory");
  std::vector<GroupHead> heads(h);
  for (int i = 0; i < h; ++i) {
    acez_trainer* t = members[i];
    GroupHead& gh = heads[i];
    memset(&gh, 0, sizeof(gh));
    // the members' own chain tables: what launch_forward / launch_dgrad hand to rowseq_kernel (a training forward)
    const std::vector<SeqLayer> f0 = forward_layers(t, t->R[0], true), f1 = forward_layers(t, t->R0_alt, true), b = dgrad_layers(t);
    for (size_t l = 0; l < f0.size(); ++l) { gh.fwd[0][l] = f0[l]; gh.fwd[1][l] = f1[l]; }
    for (size_t l = 0; l < b.size(); ++l) gh.bwd[l] = b[l];
    gh.flags = t->seq_flags; gh.spin_limit = t->seq_spin_limit;
    g->m.push_back(t);
    g->in0.push_back(t->R[0]);
    g->n_fwd = (int)f0.size(); g->n_bwd = (int)b.size();
  }
  if (hipMalloc((void**)&g->d_heads, sizeof(GroupHead) * h) != hipSuccess ||
      hipMemcpy(g->d_heads, heads.data(), sizeof(GroupHead) * h, hipMemcpyHostToDevice) != hipSuccess) {
    (void)hipGetLastError();
    acez_train_group_destroy(g);
    set_error("acez_train_group_create: device allocation failed");
    return ACEZ_ERR_HIP;
  }
  *out = g;
  return ACEZ_OK;
}

// one of the two GEMM chains of the members listed in `idx` (all of them seq_usable for their batch) as one launch per SEQ_MAX_LAYERS
// layers, with seq_account per member
template <bool BWD>
static void launch_rowseq_group(acez_train_group* g, const std::vector<int>& idx, const StepRun* runs, hipStream_t s) {
  const int total = BWD ? g->n_bwd : g->n_fwd;
  const bool f16 = g->m[0]->f16;
  for (int i0 = 0; i0 < total; i0 += SEQ_MAX_LAYERS) {
    const int cnt = std::min(SEQ_MAX_LAYERS, total - i0);
    RowSeqGroupArgs a{};
    a.heads = g->d_heads; a.H = GROUP_MAX; a.layer0 = i0; a.n_layers = cnt; a.mtiles = 0;
    // members that sit this chain out (per-layer launches) get M = 0: no row tile of theirs exists in the launch
    for (int k = 0; k < GROUP_MAX; ++k) { a.M[k] = 0; a.st[k] = nullptr; }
    a.H = (int)g->m.size();
    for (int i : idx) {
      acez_trainer* tr = g->m[i];
      a.st[i] = runs[i].st; a.M[i] = runs[i].n; a.variant[i] = tr->R[0] == g->in0[i] ? 0 : 1;
      a.mtiles = std::max(a.mtiles, row_tiles(runs[i].n));
      a.poll_bias[i] = seq_account(tr, a.base[i], runs[i].n, seq_seams(cnt), 0);   // (layers = 0: the group's chain launches open no profiling scope)
    }
    with_elt(f16, [&](auto e) { hipLaunchKernelGGL((rowseq_group_kernel<BWD, decltype(e)>), chain_grid(a.mtiles), dim3(512), 0, s, a); });
  }
}

extern "C" int acez_train_group_step(acez_train_group* g, const int64_t* const* d_indices, const int32_t* n, const int64_t* const* d_next,
                                     const int32_t* n_next, void* stream) {
  ACEZ_REQUIRE(g && d_indices && n, "null pointer");
  const int H = (int)g->m.size();
  // every argument is checked before anything is launched: a refused step changes no member
  for (int i = 0; i < H; ++i) {
    const acez_trainer* tr = g->m[i];
    ACEZ_REQUIRE(d_indices[i], "null indices");
    ACEZ_REQUIRE(tr->have_buf, "acez_trainer_set_buffer has not been called on a member");
    ACEZ_REQUIRE(n[i] > 0 && n[i] <= tr->max_batch, "n must be in [1, max_batch]");
    const int nn = (d_next && d_next[i] && n_next) ? n_next[i] : 0;
    ACEZ_REQUIRE(nn >= 0 && nn <= tr->max_batch, "n_next must be in [0, max_batch]");
  }
  ACEZ_HIP_CHECK(hipSetDevice(g->m[0]->device));
  hipStream_t s = (hipStream_t)stream;
  StepRun runs[GROUP_MAX];
  std::vector<int> chained;   // members whose chains can run as one-launch chains (seq_usable); the others take per-layer launches
  for (int i = 0; i < H; ++i) {
    const int64_t* nx = (d_next && d_next[i] && n_next) ? d_next[i] : nullptr;
    runs[i] = start_run(g->m[i], Flow::Fused, d_indices[i], n[i], nx, nx ? n_next[i] : 0, s);
    if (seq_usable(g->m[i], n[i])) chained.push_back(i);
  }
  // each member's own step phases; only the GEMM chains of the chained members run as one launch for all of them
  return run_steps(runs, H, [&](bool bwd) {
    if (!chained.empty()) (bwd ? launch_rowseq_group<true> : launch_rowseq_group<false>)(g, chained, runs, s);
    for (int i = 0; i < H; ++i)
      if (!seq_usable(g->m[i], n[i])) launch_chain(runs[i], bwd);
  });
}
