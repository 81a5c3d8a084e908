// vpath1_walk.inc -- the chase of the one-wave walk, as the text of its body: k_vpath1 (k_backtrack.hip, which says what it does and why)
// and the walk role of k_carve_v (k_carve.hip) include it, so that the chase exists once AND k_vpath1 keeps, instruction for
// instruction, the code it had when the body stood in it (as a function the same statements came out scheduled differently).
// In scope where it is included: DELTA and VP1_ROWS (compile-time; VP1_ROWS * DELTA <= 28), the logical view c, h, stride, lane = 0 .. 63,
// int x = the column on row h - 1, s_win = VP1_ROWS * 256 bytes of LDS (16-byte aligned) and the macro
//   VP1_RECORD(y_top, nrows, pe, po): after every chunk lane k holds the seam's columns pe on row y_top - 2k and po on row
//   y_top - 2k - 1, of which rows y_top .. y_top - nrows + 1 exist.
// Afterwards x is the column on row 0, which the includer records.
    constexpr int R = VP1_ROWS, NB = VP1_AHEAD + 1, RL = VP1_ROWS / 4;      // RL loads per chunk, four rows each
    // window [base, base + 256) with base in [cx - 135, cx - 120]: the 64 columns around a start column that has moved up to
    // 88 either way since the load are inside
    static_assert(VP1_ROWS % 4 == 0 && VP1_ROWS * DELTA <= 28 && VP1_AHEAD * VP1_ROWS * DELTA + 32 <= 120, "window margin");
    u32x4 regs[NB][RL];                          // ring of packed windows: chunk k lives in regs[k % NB]
    int xa[NB];                                  // their base columns
    auto window_base = [&](int cx) { return (cx - 120) & ~15; };     // multiple of 16: a lane's 16 columns never straddle column 0
    // Nothing is predicated (a select per load cost more instructions than the chase itself): columns outside
    // the plane are clamped into it -- the path never goes there -- and rows above row 1 re-read row 1; the steps
    // taken on those are discarded (see run_chunk).  Uniform row base + 32-bit lane offset: one VALU per load.
    auto load_chunk = [&](int b, int y_top, int cx) {
        const int base = window_base(cx);
        xa[b] = base;
        // lanes 16s .. 16s + 15: row y_top - 4q - s, 16 columns per lane
        const int voff = min(max(base + 16 * (lane & 15), 0), stride - 16);
        const int rsub = (lane >> 4) * stride;
#pragma unroll
        for (int q = 0; q < RL; q++) {
            const int row = max((y_top - 4 * q) * stride - rsub, stride);          // rows above row 1 re-read row 1
            regs[b][q] = *(const GLOBAL_AS u32x4 *) (c.least + (unsigned) (row + voff));
        }
    };
    // one chunk: spread the 64 columns around the start column out over the lanes, chase, record
    auto run_chunk = [&](int b, int y_top) {
        const int relbase = x - 32 - xa[b];                  // window column of lane 0's column
        int e[R];
        // through LDS: what the loads hold lane by lane IS row-major [row][256 columns]; same wave writes and reads, LDS
        // operations of a wave execute in order
#pragma unroll
        for (int q = 0; q < RL; q++) *(u32x4 *) (s_win + q * 1024 + lane * 16) = regs[b][q];
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int r = 0; r < R; r++) e[r] = s_win[r * 256 + relbase + lane];
        // two-row displacements of every column (the path stays within lanes 4 .. 60, so the wrap-around of the
        // outermost lanes' neighbours never matters)
        int e2[R / 2];
#pragma unroll
        for (int k = 0; k < R / 2; k++) e2[k] = e[2 * k] + __builtin_amdgcn_ds_bpermute((lane + e[2 * k]) << 2, e[2 * k + 1]);
        int o = 32, path = 0;
        vp1_chase<R / 2>(e2, o, path, std::make_integer_sequence<int, R / 2>{});          // lane k <- window offset at row y_top - 2k
        // the odd rows, all at once: lane k looks its even row's displacement up at the column it stands on
        const int odd = path + s_win[min(lane, R / 2 - 1) * 512 + relbase + path];
        __builtin_amdgcn_wave_barrier();
        const int pe = path + x - 32, po = odd + x - 32;     // columns at rows y_top - 2k and y_top - 2k - 1
        const int nrows = min(R, y_top);
        VP1_RECORD(y_top, nrows, pe, po);
        // the column after `nrows` steps: the last chunk may hold fewer real rows than R (the rest re-read row 1)
        x = (nrows == R) ? x + o - 32 : __builtin_amdgcn_readlane((nrows & 1) ? po : pe, nrows >> 1);
    };
    int y_top = h - 1;
    // chunks are issued VP1_AHEAD ahead; the first ones all around the argmin
#pragma unroll
    for (int k = 0; k < VP1_AHEAD; k++) load_chunk(k, y_top - k * R, x);
    while (true) {
#pragma unroll
        for (int k = 0; k < NB; k++) {
            load_chunk((k + VP1_AHEAD) % NB, y_top - VP1_AHEAD * R, x);      // in flight during this and the next two chases
            run_chunk(k, y_top);
            y_top -= R;
            if (y_top < 1) break;
        }
        if (y_top < 1) break;
    }
