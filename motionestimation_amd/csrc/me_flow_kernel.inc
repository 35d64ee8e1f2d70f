// me_flow_kernel.inc -- the flow kernel's definition, included twice by
// me_kernels.hip: ME_FLOW_CHAIN 0 gives me_flow_kernel<B, K, PC> (every launch
// without box-sum planes: it compiles none of the chain paths), ME_FLOW_CHAIN 1
// gives me_flow_chain_kernel<B, K> (the item table, flow_fill's early bound, the
// bound's peeled last chunk, one slot fill at the top of the task loop and the
// pre-bound behind its publish).  Two kernels, not one body inlined into two
// wrappers: the first must stay the code it was before the chain kernel existed.
#if ME_FLOW_CHAIN
// A pruning launch with box-sum planes (jb.planes; the 144-byte pitch).  table:
// entries of the workgroups' LDS item table behind the control block
// (flow_table_entries; 0: none, the waves decode their items themselves).
// pre: bit 0 the pre-bound on (flow_fill), bits 1-2 its issue priority.
// FlowChainArgs: the arguments as the kernel argument segment lays them out.
// INVARIANT: its members are me_flow_chain_kernel's parameters, in their order
// and with their types; the slot fill reads the launch's arguments through it
// (the task loop's top).  Whoever adds, removes or reorders a parameter edits
// both; the static_assert below the kernel holds the sizes together.
struct FlowChainArgs {
  SearchArgs p;
  QsadGeom g;
  FlowJobs jb;
  int table, pre;
};
template <int B, int K>
__global__ __launch_bounds__(1024) void me_flow_chain_kernel(SearchArgs p, QsadGeom g, FlowJobs jb, int table,
                                                             int pre) {
  // (the parameter list above is FlowChainArgs, member for member: see there)
  static_assert(std::is_same<decltype(p), decltype(FlowChainArgs::p)>::value &&
                    std::is_same<decltype(g), decltype(FlowChainArgs::g)>::value &&
                    std::is_same<decltype(jb), decltype(FlowChainArgs::jb)>::value &&
                    std::is_same<decltype(table), decltype(FlowChainArgs::table)>::value &&
                    std::is_same<decltype(pre), decltype(FlowChainArgs::pre)>::value &&
                    offsetof(FlowChainArgs, pre) + sizeof(int) == sizeof(FlowChainArgs),
                "FlowChainArgs mirrors this kernel's parameters");
  constexpr int PC = 144;
  [[maybe_unused]] constexpr bool CHAIN = true;
#else
template <int B, int K, int PC>
__global__ __launch_bounds__(1024) void me_flow_kernel(SearchArgs p, QsadGeom g, FlowJobs jb) {
  [[maybe_unused]] constexpr bool CHAIN = false;
  [[maybe_unused]] constexpr int table = 0;
#endif
  static_assert(B == 16, "cur-block DMA layout of stage_item_wave");
  constexpr int CW = B / 4;
  extern __shared__ __align__(16) uint8_t smem[];
  // Pruning (flow_bound above) is compiled into the 144-byte-pitch instance
  // only: the planner turns it on for no other shape.
  const bool prune = PC == 144 && g.prune != 0;
  // (a pruning launch with box-sum planes: the slim bound scratch, more slots)
  const bool slim = prune && jb.planes != nullptr;
  const int NB = !prune ? g.flow_slots : slim ? g.slim_slots : g.prune_slots;
  const int slot_bytes = g.tile_bytes + g.tb * B * B + (!prune ? 0 : slim ? FLOW_SLIM_BYTES : FLOW_PRUNE_BYTES);
  uint64_t* keys = reinterpret_cast<uint64_t*>(smem + NB * slot_bytes);  // [NB][tb]
  FlowCtl* ctl = reinterpret_cast<FlowCtl*>(smem + NB * slot_bytes + NB * g.tb * 8);
  const int tid = (int)threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int S = p.range;

  // This workgroup's tiles: the XCD band of bid % 8 (a speed heuristic only),
  // member m takes tiles band0 + m, + n_x, ... (every job's tiles, job-major)
  const int ntiles = jb.tile_pre[jb.n];
#if ME_FLOW_CHAIN
  const int bid = (int)blockIdx.x;
  const FlowWalk walk = flow_walk(ntiles, (int)gridDim.x, bid);
  const int nitems = walk.nitems;
  auto tile_of = [&](int k) { return walk.tile0 + k * walk.step; };
#else  // (flow_walk of me_geom.h written out, as this kernel always had it)
  const int nwg = (int)gridDim.x, bid = (int)blockIdx.x;
  const int ng = nwg < 8 ? nwg : 8;
  const int x = bid % ng, m = bid / ng;
  const int n_x = nwg / ng + (x < nwg % ng ? 1 : 0);
  const int band0 = (int)((long)ntiles * x / ng), band1 = (int)((long)ntiles * (x + 1) / ng);
  const int nitems = band1 - band0 > m ? (band1 - band0 - m + n_x - 1) / n_x : 0;
  auto tile_of = [&](int k) { return band0 + m + k * n_x; };
#endif
#if ME_FLOW_CHAIN
  // The item table (me_geom.h FlowEntry) behind the control block of a launch
  // with planes, where the host found room for it: entries 0 .. nitems.
  // (tabled0: for the code in front of the task loop, which reads PF_TABLE)
  const bool tabled0 = slim && table > 0;
  FlowEntry* tab = reinterpret_cast<FlowEntry*>(reinterpret_cast<uint8_t*>(ctl) + FLOW_CTL_BYTES);
#endif

  if (tid < 64) {
    if (tid == 0) ctl->next = 0;
    if (tid < 16) {
      ctl->ready[tid] = 0;
      ctl->done[tid] = 0;
      if (prune) ctl->live[tid] = 0;
    }
    if (prune && tid >= 32 && tid < 36) ctl->stats[tid - 32] = 0;
    if (prune && tid >= 36 && tid < 39) ctl->split[tid - 36] = 0;
    // (tuning build: executed wave-tasks of h = B items by list entries held, 64 counters behind the block
    // and the table; their place is kept in the block, so the task loop holds no argument or pointer for them)
    if (prune && g.prune_stats == 2) {
      const uint32_t off = (uint32_t)(FLOW_CTL_BYTES + table * FLOW_ENTRY_BYTES);
      reinterpret_cast<uint32_t*>(reinterpret_cast<uint8_t*>(ctl) + off)[tid] = 0;
      if (tid == 0) ctl->hist_off = off;
    }
#if ME_FLOW_CHAIN
    if (tid >= 39 && tid < 42) ctl->pre[tid - 39] = 0;
#endif
    if (tid == 16) {
      ctl->run = 0;
      ctl->pflags = !prune ? 0u
                           : (uint32_t)(PF_ON | (g.prune == 2 ? PF_VERIFY : 0) | (g.prune_bypass ? PF_BYPASS : 0) |
                                        (g.prune_stats ? PF_STATS : 0) | (jb.planes ? PF_PLANES : 0) |
#if ME_FLOW_CHAIN
                                        // (every item's window is rows_alloc rows: g.tile_bytes = it.prows * g.pitch,
                                        // the bytes stage_item_wave's steps cover, because cpp == chunks in a flow plan)
                                        (tabled0 ? PF_TABLE : 0) |
                                        (slim && (pre & 1) ? PF_PRE | ((pre >> 1) & 3) << PF_PRE_PRIO_SHIFT : 0) |
                                        (slim && g.cpp == g.chunks && g.tile_bytes > (FLOW_WIN_STEPS - 1) * 1024 &&
                                                 g.tile_bytes <= FLOW_WIN_STEPS * 1024
                                             ? PF_EARLY
                                             : 0) |
#endif
                                        (g.prune_split ? PF_SPLIT : 0) | (g.prune_split == 2 ? PF_SPLIT_124 : 0) |
                                        (g.prune_stats == 2 ? PF_HIST : 0));
    }
  }
  for (int i = tid; i < NB * g.tb; i += (int)blockDim.x) keys[i] = ~0ull;
#if ME_FLOW_CHAIN
  {
    if (tabled0) {
      // Every item decoded once, a thread each: the job by bisection of a copy
      // of tile_pre in LDS (slot 0 is free until the start ring; indexing the
      // argument arrays by lane would copy them to scratch), its task count into
      // `pre`; then wave 0 turns the counts into exclusive prefixes.
      constexpr int JR0 = MAX_JOBS + 1;        // r0 behind the MAX_JOBS + 1 tile_pre entries
      int* jt = reinterpret_cast<int*>(smem);  // [0 .. MAX_JOBS] tile_pre, [JR0 ..] r0
      if (tid == 0) {
#pragma unroll
        for (int i = 0; i <= MAX_JOBS; i++) jt[i] = jb.tile_pre[i];
#pragma unroll
        for (int i = 0; i < MAX_JOBS; i++) jt[JR0 + i] = jb.r0[i];
      }
      __syncthreads();
      for (int k = tid; k < nitems; k += (int)blockDim.x) {
        const int tile = tile_of(k);
        const int j = flow_job_find_in(jt, jb.n, tile);
        const uint32_t pack = flow_entry_of(g, tile, j, jt[j], jt[JR0 + j]);
        int lc0;
        tab[k].pack = pack;
        tab[k].pre = (uint32_t)flow_item_tasks(p, g, K, flow_entry_item(p, g, B, K, pack), &lc0);
      }
      __syncthreads();
      if (wave == 0) {
        uint32_t base = 0;
        for (int k0 = 0; k0 <= nitems; k0 += 64) {
          const int k = k0 + lane;
          const uint32_t c = k < nitems ? tab[k].pre : 0u;
          uint32_t inc = c;
#pragma unroll
          for (int d = 1; d < 64; d <<= 1) {
            const uint32_t o = (uint32_t)__shfl_up((int)inc, d);
            if (lane >= d) inc += o;
          }
          if (k <= nitems) tab[k].pre = base + inc - c;
          base += (uint32_t)__shfl((int)inc, 63);
        }
      }
    }
  }
#endif
  __syncthreads();
#if ME_FLOW_CHAIN
  // Wave w < NB stages item w and publishes it, by the one copy of the slot
  // fill this kernel has: at the top of the task loop, where the wave that ran
  // an item's last task also arrives with the slot's next item (kfill in slot
  // sfill).  Staggered as below.
  int kfill = -1, sfill = 0;
  if (wave < NB && wave < nitems) {
    for (int i = 0; i < wave; i++) __builtin_amdgcn_s_sleep(10);
    kfill = sfill = wave;
  }
#else
  // wave w < NB stages item w and publishes it
  if (wave < NB && wave < nitems) {
    // Staggered start (wave w waits w x 640 cycles): item 0's DMA gets the
    // CU's memory pipeline first and lands early instead of every item
    // landing together at the end of one burst (1080p, same box:
    // 78.4 -> 78.0 us; with the compile-time pitch 79.0 -> 77.3,
    // profiles/r02ae_ab_flow_start.txt).
    for (int i = 0; i < wave; i++) __builtin_amdgcn_s_sleep(10);
    if (g.prio) __builtin_amdgcn_s_setprio(3);  // see me_fast_kernel
    const Item it0 = flow_item<B, K>(p, g, jb, tile_of(wave), -1);
    stage_item_wave<B>(p, g, it0, smem + wave * slot_bytes, jb);
    if constexpr (PC == 144) {
      // (the bound's first plane rows: issued here, landed by the same wait)
      FlowPlaneRegs R;
      const bool pl0 = prune && flow_plane_wanted<B>(it0, ctl);
      if (pl0) flow_plane_fetch<B, K>(it0, jb, R);
      else flow_plane_zero(R);
      if (g.prio) __builtin_amdgcn_s_setprio(0);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      if (prune)
        flow_bound<B, K>(p, g, it0, smem + wave * slot_bytes, keys + wave * g.tb, ctl, wave, jb, R, pl0);
    } else {
      if (g.prio) __builtin_amdgcn_s_setprio(0);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
#ifdef ME_STAMPS
    if (lane == 0 && (int)blockIdx.x < (1 << 12)) {
      g_first[(int)blockIdx.x * 16 + wave] = ~0ull;
      g_pub[(int)blockIdx.x * 16 + wave] = __builtin_amdgcn_s_memtime();
    }
#endif
    if (lane == 0)
      __hip_atomic_store(&ctl->ready[wave], (uint32_t)wave + 1u, __ATOMIC_RELEASE,
                         __HIP_MEMORY_SCOPE_WORKGROUP);
  }
#endif

  int kc = 0, basec = 0, lc0c = 0, nwc = 0;  // this wave's view: item kc's first task, task count
  Item itc;
  bool have = false;
#ifdef ME_STAMPS
  // diagnostic build: per wave [start, first task, loop exit, spin cycles, tasks,
  // realtime start, realtime end, hw_id | ring slots << 32] (tools/flow_stamps.py)
  const int fw = bid * 16 + wave;
  unsigned long long st_t0 = __builtin_amdgcn_s_memtime(), st_first = 0, st_spin = 0, st_n = 0;
  const unsigned long long st_r0 = __builtin_amdgcn_s_memrealtime();
  unsigned long long st_dma = 0, st_bound = 0, st_nb = 0;  // refills: DMA wait, bound phase, count
  // executed wave-tasks run with 1, 2, 4 lanes per list entry: count << 40 | cycles (list read to key merge)
  unsigned long long st_k1 = 0, st_k2 = 0, st_k4 = 0;
  // the tile -> item decode (flow_item) at the advance and at the refill: count << 40 | cycles
  unsigned long long st_da = 0, st_dr = 0;
  unsigned long long st_pt = 0, st_pn = 0;  // publish -> first executed task: cycles, items
  // the bound's split (g_bstamps); [8], [9]: the chain kernel's post-bounds' waits on BUSY, cycles and count
  unsigned long long st_b[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  // the chain kernel: pre-bounds (cycles, count), last task done -> publish of the refills (cycles; st_nb counts them)
  unsigned long long st_pre = 0, st_pren = 0, st_rp = 0, st_last = 0;
#define ME_DECODE_T0 const unsigned long long st_i0 = __builtin_amdgcn_s_memtime()
#define ME_DECODE_T1(acc, item)                                                   \
  do {                                                                            \
    asm volatile("" ::"s"((item).j), "s"((item).by), "s"((item).bx0));            \
    (acc) += (1ull << 40) + (__builtin_amdgcn_s_memtime() - st_i0);               \
  } while (0)
#else
#define ME_DECODE_T0
#define ME_DECODE_T1(acc, item)
#endif
  for (;;) {
    const int pfl = PC == 144 ? __builtin_amdgcn_readfirstlane((int)ctl->pflags) : 0;
#if ME_FLOW_CHAIN
    if (kfill >= 0) {
      // Fill slot sfill with item kfill and publish it; then the pre-bound of
      // the slot's next item (flow_fill's comment has the marker's protocol).
      const int kn = kfill, slotn = sfill;
      // The fill reads the launch's arguments through a pointer to the kernel
      // argument segment that the compiler cannot follow out of the loop: what
      // it derives from the arguments themselves is all formed in front of the
      // task loop and held across it, in SGPRs the loop has to spill.
      typedef const __attribute__((address_space(4))) FlowChainArgs* ArgPtr;
      ArgPtr ka = (ArgPtr)__builtin_amdgcn_kernarg_segment_ptr();
      asm volatile("" : "+s"(ka));
      const SearchArgs& pa = *(const SearchArgs*)&ka->p;
      const QsadGeom& ga = *(const QsadGeom*)&ka->g;
      const FlowJobs& ja = *(const FlowJobs*)&ka->jb;
      uint8_t* bufn = smem + slotn * slot_bytes;
      if (ga.prio) __builtin_amdgcn_s_setprio(3);  // see me_fast_kernel
      ME_DECODE_T0;
      // (kn > kc: the job of this wave's current item is not behind kn's)
      const Item itn = (pfl & PF_TABLE)
                           ? flow_entry_item(pa, ga, B, K, (uint32_t)__builtin_amdgcn_readfirstlane((int)tab[kn].pack))
                           : flow_item<B, K>(pa, ga, ja, tile_of(kn), have ? itc.j : -1);
      ME_DECODE_T1(st_dr, itn);
      bool expired = false;
#ifdef ME_STAMPS
      const unsigned long long st_d0 = __builtin_amdgcn_s_memtime();
      unsigned long long st_d1 = 0;
      flow_fill<B, K>(pa, ga, itn, bufn, keys + slotn * ga.tb, ctl, slotn, ja, pfl, kn >= NB, kn, NB, &expired, &st_d1,
                      kn >= NB ? st_b : nullptr);
      if (kn >= NB) {
        st_dma += st_d1 - st_d0;
        st_bound += __builtin_amdgcn_s_memtime() - st_d1;
        st_nb++;
      }
#else
      flow_fill<B, K>(pa, ga, itn, bufn, keys + slotn * ga.tb, ctl, slotn, ja, pfl, kn >= NB, kn, NB, &expired, nullptr);
#endif
      if (expired) break;
      // the marker of this turn: whether item kn + NB is pre-bound behind the publish
      const int kp = kn + NB;
      bool prb = (pfl & PF_PRE) && kp < nitems;
      if (prb && (pfl & PF_BYPASS))
        prb = __builtin_amdgcn_readfirstlane(
                  (int)__hip_atomic_load(&ctl->run, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) < 4;
      Item itp = itn;
      if (prb) {
        itp = (pfl & PF_TABLE)
                  ? flow_entry_item(pa, ga, B, K, (uint32_t)__builtin_amdgcn_readfirstlane((int)tab[kp].pack))
                  : flow_item<B, K>(pa, ga, ja, tile_of(kp), itn.j);
        prb = itp.h == B;
      }
      uint32_t* mark = flow_mark_of<B>(ga, bufn);
      if ((pfl & PF_PRE) && lane == 0)
        __hip_atomic_store(mark, prb ? flow_mark_busy(kp) : FLOW_MARK_NONE, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_WORKGROUP);
#ifdef ME_STAMPS
      if (lane == 0 && bid < (1 << 12)) {
        g_first[bid * 16 + slotn] = ~0ull;
        g_pub[bid * 16 + slotn] = __builtin_amdgcn_s_memtime();
      }
      if (kn >= NB) st_rp += __builtin_amdgcn_s_memtime() - st_last;
#endif
      if (lane == 0)
        __hip_atomic_store(&ctl->ready[slotn], (uint32_t)kn + 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
      if (prb) {
#ifdef ME_STAMPS
        const unsigned long long st_p0 = __builtin_amdgcn_s_memtime();
#endif
        // (off the chain unless it is late: the issue priority the launch names)
        const int pp = (pfl & PF_PRE_PRIO) >> PF_PRE_PRIO_SHIFT;
        if (pp == 3) __builtin_amdgcn_s_setprio(3);
        else if (pp == 1) __builtin_amdgcn_s_setprio(1);
        flow_prebound<B, K>(pa, ga, itp, bufn, keys + slotn * ga.tb, ctl, slotn, ja);
        __builtin_amdgcn_s_setprio(0);
        if (lane == 0) {
          __hip_atomic_store(mark, flow_mark_done(kp), __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
          if (pfl & PF_STATS) atomicAdd(&ctl->pre[0], 1u);
        }
#ifdef ME_STAMPS
        st_pre += __builtin_amdgcn_s_memtime() - st_p0;
        st_pren++;
#endif
      }
    }
#endif
    uint32_t q = 0;
    if (lane == 0) q = __hip_atomic_fetch_add(&ctl->next, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    q = (uint32_t)__builtin_amdgcn_readfirstlane((int)q);
    // advance to the item holding task q (pulls are in order: kc only grows)
#if ME_FLOW_CHAIN
    const bool tabled = (pfl & PF_TABLE) != 0;
    if (tabled) {
      // From the table: the prefixes of the next 64 items in one LDS read, the
      // items task q has passed counted by a ballot (prefixes only grow; entry
      // nitems holds the workgroup's task count and repeats in the lanes past it).
      if (!have || (int)q >= basec + nwc) {
        const int fl = fresh_tid() & 63;  // (no lane-derived table address kept across the task loop)
        for (;;) {
          const int idx = min(kc + 1 + fl, nitems);
          const int adv = (int)__builtin_popcountll(__builtin_amdgcn_ballot_w64(q >= tab[idx].pre));
          kc += adv;
          if (adv < 64 || kc >= nitems) break;
        }
        if (kc < nitems) {
          ME_DECODE_T0;
          const uint32_t pack = (uint32_t)__builtin_amdgcn_readfirstlane((int)tab[kc].pack);
          basec = __builtin_amdgcn_readfirstlane((int)tab[kc].pre);
          itc = flow_entry_item(p, g, B, K, pack);
          nwc = flow_item_tasks(p, g, K, itc, &lc0c);
          ME_DECODE_T1(st_da, itc);
          have = true;
        }
      }
    } else
#endif
    if (!have && kc < nitems) {
      ME_DECODE_T0;
      itc = flow_item<B, K>(p, g, jb, tile_of(kc), -1);
      ME_DECODE_T1(st_da, itc);
      nwc = flow_tasks<B, K>(p, g, itc, &lc0c);
      have = true;
    }
    while (kc < nitems && (int)q >= basec + nwc) {
      basec += nwc;
      kc++;
      if (kc < nitems) {
        ME_DECODE_T0;
        itc = flow_item<B, K>(p, g, jb, tile_of(kc), itc.j);  // (kc grew: its job did not fall)
        ME_DECODE_T1(st_da, itc);
        nwc = flow_tasks<B, K>(p, g, itc, &lc0c);
      }
    }
    if (kc >= nitems) break;
    if (g.fair) __builtin_amdgcn_s_setprio(0);
    const int slot = kc % NB;
    // Bounded wait (the ordering argument above says it ends; the bound keeps a
    // broken invariant from hanging the GPU).  An expired wait is reported:
    // sched[SCHED_ERR] is set, and the host turns it into ME_EDEVICE
    // (device_status after the synchronous entry points, me_device_check).
    int spins = 0;
#ifdef ME_STAMPS
    const unsigned long long st_w0 = __builtin_amdgcn_s_memtime();
#endif
    while (__hip_atomic_load(&ctl->ready[slot], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) !=
               (uint32_t)kc + 1u &&
           ++spins < (1 << 20))
      __builtin_amdgcn_s_sleep(2);
    if (spins >= (1 << 20)) {
      if (lane == 0 && p.sched)
        __hip_atomic_store(p.sched + SCHED_ERR, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      break;
    }
#ifdef ME_STAMPS
    {
      const unsigned long long now = __builtin_amdgcn_s_memtime();
      st_spin += now - st_w0;
      if (!st_first) st_first = now;
      st_n++;
    }
#endif
    const Item& it = itc;
    uint8_t* buf = smem + slot * slot_bytes;
    const uint32_t* cur_lds = reinterpret_cast<const uint32_t*>(buf + g.tile_bytes);
    const uint32_t tile_off = (uint32_t)(slot * slot_bytes);
    const int G = g.groups;
    const int t = (int)q - basec;
    const int dymin = max(-S, -it.tly), dymax = min(S, p.height - it.h - it.tly);
    const int lc1 = min(it.nch, (dymax + S) / K + 1);
    const int valid_lanes = (lc1 - lc0c) * it.nb * G;
    // Pruning: task t takes the item's live lane-tasks [64 t, 64 t + 64) of the
    // slot's list; a task past the list only counts itself done.
    const int nlive = pfl ? __builtin_amdgcn_readfirstlane((int)ctl->live[slot]) : valid_lanes;
    if (64 * t < nlive) {
    // Fairness: the SIMD arbiter issues the oldest waves first, so a young
    // wave's wave-task lags while older waves run through later items (single
    // 1080p frames: per SIMD one wave ran ~6 wave-tasks, two ran 1 each), and
    // the slot refill that waits for it stalls every wave behind the ring.
    // Every 4 rows the wave compares its task with the pull counter and raises
    // its priority once lo / hi later tasks have been pulled (g.fair; back to
    // 0 at its next pull).  Only in launches with refills: without them (a
    // single 1080p frame, every tile staged at the start) the oldest-first
    // order ends the launch sooner (70.4 vs 74.7 us with the check on,
    // profiles/r03ad_*).  Tuning build, g.fair bits 16-17 (ME_FAIR): 2 = only
    // on items whose slot still gets a refill, 3 = on every item.
    const int fmode = g.fair >> 16;
    const bool fair = g.fair != 0 && (fmode == 3 || (fmode == 2 ? kc + NB < nitems : nitems > NB));
    // pull-counter values that raise the priority (two SGPRs across the rows)
    const int lim1 = __builtin_amdgcn_readfirstlane(fair ? (int)q + (g.fair & 255) : 0x7FFFFFFF);
    const int lim2 = __builtin_amdgcn_readfirstlane(fair ? (int)q + ((g.fair >> 8) & 255) : 0x7FFFFFFF);
    // The compare and s_setprio sit in one asm block: as C branches they split
    // the unrolled row loop into basic blocks, and it spilled 41 VGPRs.
    auto lag_check = [lim1, lim2, ctl]() {
      const int nx = __builtin_amdgcn_readfirstlane(
          (int)__hip_atomic_load(&ctl->next, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
      asm volatile(
          "s_cmp_ge_i32 %0, %2\n\t"
          "s_cbranch_scc0 1f\n\t"
          "s_setprio 2\n\t"
          "s_branch 2f\n"
          "1:\n\t"
          "s_cmp_ge_i32 %0, %1\n\t"
          "s_cbranch_scc0 2f\n\t"
          "s_setprio 1\n"
          "2:" ::"s"(nx), "s"(lim1), "s"(lim2) : "scc");
    };
    // The rows a lane of the task takes: K runs it whole (below), 7, 4, 3, 2
    // and 1 split it over 2, 4, 5, 7 and 13 lanes per list entry
    // (flow_split_task; pruned h = B items only: an h = B/2 item's list is
    // full).  cls: the counters' class, whole / 2 / 4 or more lanes per entry.
    int rows = K;
#ifdef ME_STAMPS
    const unsigned long long st_k0 = __builtin_amdgcn_s_memtime();
    if (lane == 0 && bid < (1 << 12)) atomicMin(&g_first[bid * 16 + slot], st_k0);
#endif
    if constexpr (PC == 144) {
      const int n = nlive - 64 * t;
      if ((pfl & PF_SPLIT) && it.h == B && n <= 32)
        rows = (pfl & PF_SPLIT_124) ? flow_split_rows_124(n) : flow_split_rows(n);
      if ((pfl & PF_STATS) && lane == 0) {
        atomicAdd(&ctl->split[rows == K ? 0 : rows == 7 ? 1 : 2], 1u);
        if ((pfl & PF_HIST) && it.h == B)
          atomicAdd(reinterpret_cast<uint32_t*>(reinterpret_cast<uint8_t*>(ctl) + ctl->hist_off) + min(n, 64) - 1, 1u);
      }
#define ME_SPLIT_TASK(R) \
  flow_split_task<B, K, PC, R>(p, g, it, smem, buf, tile_off, keys + slot * g.tb, t, n, lc0c, pfl, lag_check)
      if (rows == 1) ME_SPLIT_TASK(1);
      else if (rows == 2) ME_SPLIT_TASK(2);
      else if (rows == 3) ME_SPLIT_TASK(3);
      else if (rows == 4) ME_SPLIT_TASK(4);
      else if (rows == 7) ME_SPLIT_TASK(7);
#undef ME_SPLIT_TASK
    }
#ifdef ME_STAMPS
    const int cls = rows == K ? 0 : rows == 7 ? 1 : 2;
#endif
    if (rows == K) {
    const bool live = 64 * t + lane < nlive;
    const uint16_t* llist = reinterpret_cast<const uint16_t*>(buf + g.tile_bytes + g.tb * B * B);
    const int i = pfl && live ? (int)llist[64 * t + lane] : 64 * t + lane;
    const int ii = live ? i : 0;
    const int bg = (int)__umulhi((uint32_t)ii, g.magic_groups);  // ii / G
    const int gi = ii - bg * G;
    const uint32_t magic_nb = 0xFFFFFFFFu / (uint32_t)it.nb + 1u;
    const int lcr = it.nb == 1 ? bg : (int)__umulhi((uint32_t)bg, magic_nb);
    const int b = bg - lcr * it.nb;
    const int lc = lc0c + lcr;
    const int d0 = lc * K;
    const int tlx = (it.bx0 + b) * B;
    uint32_t c[B][CW];
#pragma unroll
    for (int y = 0; y < B; y++) {
      if constexpr (CW == 4) {
        const uint4 v = reinterpret_cast<const uint4*>(cur_lds)[b * B + y];
        c[y][0] = v.x; c[y][1] = v.y; c[y][2] = v.z; c[y][3] = v.w;
      } else {
        const uint2 v = reinterpret_cast<const uint2*>(cur_lds)[b * B + y];
        c[y][0] = v.x; c[y][1] = v.y;
      }
    }
    const int dxmin = max(-S, -tlx), dxmax = min(S, p.width - B - tlx);
    const int jlo = dymin + S - d0, jhi = dymax + S - d0;
    const bool full_rows = dymin + S <= 0 && dymax + S >= it.nch * K - 1;
    const int w0 = (b * B) / 4 + gi;
    uint64_t acc[K];
    const int jt = gi < K ? gi : K - 1;
    const uint32_t toff = tile_off + (uint32_t)((lc * K + jt) * g.pitch + b * B + 2 * S);
    uint32_t tsad = 0;
    if (it.h == B) {
      qsad_lane<B, K, B, PC, 4>(smem, g.pitch, tile_off, lc * K, w0, c, acc, lag_check);
      if (g.fold) tsad = tail_sad<B, B>(smem, g.pitch, toff, c);
    } else {
      qsad_lane<B, K, B / 2, PC, 4>(smem, g.pitch, tile_off, lc * K, w0, c, acc, lag_check);
      if (g.fold) tsad = tail_sad<B, B / 2>(smem, g.pitch, toff, c);
    }
    const int dxg = 4 * gi - S - it.a;
    const bool edge = dxg < dxmin || dxg + 3 > dxmax || !live;
    uint32_t best;
    if (full_rows && __builtin_amdgcn_ballot_w64(edge) == 0) {
      best = lane_best<K, false>(acc, 0u, 0u, jlo, jhi);
    } else {
      uint32_t mlo = 0, mhi = 0;
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const int dx = dxg + k;
        const uint32_t msk = (dx < dxmin || dx > dxmax) ? 0xFFFFu : 0u;
        if (k < 2) mlo |= msk << (16 * k);
        else mhi |= msk << (16 * (k - 2));
      }
      best = lane_best<K, true>(acc, mlo, mhi, jlo, jhi);
    }
    if (g.fold) {
      const bool tv = gi < K && jt >= jlo && jt <= jhi && S <= dxmax;
      best = min(best, tv ? (tsad << 16) | (uint32_t)(5 * jt + 4) : ~0u);
    }
    if (live && best < 0xFFFF0000u) {
      const int idx = (int)(best & 0xFFFFu), jj = idx / 5, k5 = idx - 5 * jj;
      const int dy = d0 + jj - S, dx = k5 == 4 ? S : 4 * gi + k5 - S - it.a;
      atomicMin(reinterpret_cast<unsigned long long*>(&keys[slot * g.tb + b]),
                (unsigned long long)make_key(best >> 16, dx, dy));
    }
    if constexpr (PC == 144) {
      // Verify mode: a lane-task the bound marked dead must hold no candidate
      // with SAD <= its block's U_b.
      if ((pfl & PF_VERIFY) && live && best < 0xFFFF0000u) {
        const uint8_t* pv = buf + g.tile_bytes + g.tb * B * B;
        if (pv[FLOW_PRUNE_DEAD + i] && (best >> 16) <= reinterpret_cast<const uint32_t*>(pv + FLOW_PRUNE_UB)[b] && p.sched)
          __hip_atomic_store(p.sched + SCHED_ERR, 2u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
    }
#ifdef ME_STAMPS
    {  // executed wave-tasks per class: count << 40 | cycles
      const unsigned long long dt = (1ull << 40) + (__builtin_amdgcn_s_memtime() - st_k0);
      st_k1 += cls == 0 ? dt : 0;
      st_k2 += cls == 1 ? dt : 0;
      st_k4 += cls == 2 ? dt : 0;
    }
#endif
    }
    // this wave-task is done; the last one of the item writes and refills the slot
#if ME_FLOW_CHAIN
    kfill = -1;
#endif
    uint32_t prev = 0;
    if (lane == 0)
      prev = __hip_atomic_fetch_add(&ctl->done[slot], 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_WORKGROUP);
    prev = (uint32_t)__builtin_amdgcn_readfirstlane((int)prev);
    if ((int)prev + 1 == nwc) {
#ifdef ME_STAMPS
      st_last = __builtin_amdgcn_s_memtime();
      if (bid < (1 << 12)) {  // (every task of the item is done: its earliest start stands)
        const unsigned long long f = __hip_atomic_load(&g_first[bid * 16 + slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const unsigned long long pb = __hip_atomic_load(&g_pub[bid * 16 + slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (f != ~0ull && pb && f >= pb) {
          st_pt += f - pb;
          st_pn++;
        }
      }
#endif
      if (lane < it.nb) {
        const uint64_t kk = keys[slot * g.tb + lane];
        uint64_t none = ~0ull;  // materialised here, not kept live (it spilled)
        asm volatile("" : "+v"(none));
        keys[slot * g.tb + lane] = none;
        const int out = (it.by - jb.r0[it.j]) * p.nbx + it.bx0 + lane;
        int16_t* mv = jb.mv[it.j];
        store_mv(mv, out, kk);
        if (jb.cost[it.j]) jb.cost[it.j][out] = (uint32_t)(kk >> 32);
      }
      if (lane == 0) __hip_atomic_store(&ctl->done[slot], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      const int kn = kc + NB;
#if ME_FLOW_CHAIN
      // (the slot's next item: filled and published at the top of the loop)
      if (kn < nitems) {
        kfill = kn;
        sfill = slot;
      }
#else
      if (kn < nitems) {
        if (g.prio) __builtin_amdgcn_s_setprio(3);
        ME_DECODE_T0;
        const Item itn = flow_item<B, K>(p, g, jb, tile_of(kn), it.j);  // (kn > kc)
        ME_DECODE_T1(st_dr, itn);
#ifdef ME_STAMPS
        const unsigned long long st_d0 = __builtin_amdgcn_s_memtime();
#endif
        stage_item_wave<B>(p, g, itn, buf, jb);
        if constexpr (PC == 144) {
          FlowPlaneRegs R;
          const bool pln = pfl && flow_plane_wanted<B>(itn, ctl);
          if (pln) flow_plane_fetch<B, K>(itn, jb, R);
          else flow_plane_zero(R);
          if (g.prio) __builtin_amdgcn_s_setprio(0);
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#ifdef ME_STAMPS
          const unsigned long long st_d1 = __builtin_amdgcn_s_memtime();
          st_dma += st_d1 - st_d0;
          st_bound -= st_d1;
#endif
          // (at raised issue priority: nothing of the item runs before its bound ends)
          if (pfl) {
            __builtin_amdgcn_s_setprio(3);
#ifdef ME_STAMPS
            flow_bound<B, K>(p, g, itn, buf, keys + slot * g.tb, ctl, slot, jb, R, pln, st_b);
#else
            flow_bound<B, K>(p, g, itn, buf, keys + slot * g.tb, ctl, slot, jb, R, pln);
#endif
            __builtin_amdgcn_s_setprio(0);
          }
        } else {
          if (g.prio) __builtin_amdgcn_s_setprio(0);
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#ifdef ME_STAMPS
          const unsigned long long st_d1 = __builtin_amdgcn_s_memtime();
          st_dma += st_d1 - st_d0;
          st_bound -= st_d1;
#endif
        }
#ifdef ME_STAMPS
        st_bound += __builtin_amdgcn_s_memtime();
        st_nb++;
#endif
#ifdef ME_STAMPS
        if (lane == 0 && bid < (1 << 12)) {
          g_first[bid * 16 + slot] = ~0ull;
          g_pub[bid * 16 + slot] = __builtin_amdgcn_s_memtime();
        }
#endif
        if (lane == 0)
          __hip_atomic_store(&ctl->ready[slot], (uint32_t)kn + 1u, __ATOMIC_RELEASE,
                             __HIP_MEMORY_SCOPE_WORKGROUP);
      }
#endif
    }
  }
  if constexpr (PC == 144) {
    // Tuning build: this workgroup's counts, once every wave is out of the loop.
    if ((__builtin_amdgcn_readfirstlane((int)ctl->pflags) & PF_STATS) && p.sched) {
      __syncthreads();
      if (tid < 4) atomicAdd(p.sched + SCHED_PRUNE + tid, ctl->stats[tid]);
      if (tid >= 4 && tid < 7) atomicAdd(p.sched + SCHED_SPLIT + tid - 4, ctl->split[tid - 4]);
      if ((ctl->pflags & PF_HIST) && tid >= 64 && tid < 128) {
        const uint32_t v = reinterpret_cast<uint32_t*>(reinterpret_cast<uint8_t*>(ctl) + ctl->hist_off)[tid - 64];
        if (v) atomicAdd(p.sched + SCHED_SPLIT_HIST + tid - 64, v);
      }
#if ME_FLOW_CHAIN
      if (tid >= 7 && tid < 10) atomicAdd(p.sched + SCHED_PRE + tid - 7, ctl->pre[tid - 7]);
#endif
    }
  }
#ifdef ME_STAMPS
  if (lane == 0 && fw < (1 << 16)) {
    unsigned hw;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
    unsigned long long* o = g_stamps + 8 * fw;
    o[0] = st_t0; o[1] = st_first; o[2] = __builtin_amdgcn_s_memtime(); o[3] = st_spin;
    o[4] = st_n; o[5] = st_r0; o[6] = __builtin_amdgcn_s_memrealtime();
    o[7] = hw | (unsigned long long)NB << 32;  // (the launch's ring slots above the hw id)
    // per wave, refills: [DMA wait cycles, bound cycles, refills]; executed
    // wave-tasks by class: [whole, 2, 4 lanes per entry] as count << 40 | cycles;
    // flow_item decodes at [the advance, the refill] likewise
    if (fw < (1 << 14)) {
      g_wstamps[8 * fw] = st_dma; g_wstamps[8 * fw + 1] = st_bound; g_wstamps[8 * fw + 2] = st_nb;
      g_wstamps[8 * fw + 3] = st_k1; g_wstamps[8 * fw + 4] = st_k2; g_wstamps[8 * fw + 5] = st_k4;
      g_wstamps[8 * fw + 6] = st_da; g_wstamps[8 * fw + 7] = st_dr;
#pragma unroll
      for (int i = 0; i < 8; i++) g_bstamps[16 * fw + i] = st_b[i];
      g_bstamps[16 * fw + 8] = st_pt; g_bstamps[16 * fw + 9] = st_pn;
      // the chain kernel: waits on BUSY [cycles, count], pre-bounds [cycles, count], last task done -> publish of the refills
      g_bstamps[16 * fw + 10] = st_b[8]; g_bstamps[16 * fw + 11] = st_b[9];
      g_bstamps[16 * fw + 12] = st_pre; g_bstamps[16 * fw + 13] = st_pren; g_bstamps[16 * fw + 14] = st_rp;
    }
  }
#endif
#undef ME_DECODE_T0
#undef ME_DECODE_T1
}
