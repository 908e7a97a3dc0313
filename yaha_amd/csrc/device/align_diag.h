// align_diag.h -- the diagnostics of the align stage (stage_align.hip, which alone includes this header, behind its kernel headers): host code that copies device
// arrays back and prints what it finds on stderr.  Each is called behind YGPU_TRACE (and its own switch) at the point of the stream it looks at;
// the two profile functions do something only in the YD_PROF build.  None of them is part of the pipeline: they launch nothing and change no buffer of a batch.
#pragma once

// YGPU_JOINT_HIST: the DP joints by kernel class and shape (which kernel takes what: gapJointKey)
static void diagJointHist(ygpu_ctx *ctx, uint32_t J)
{
    std::vector<JointRec> hj(J); hipMemcpy(hj.data(), ctx->joints.p, sizeof(JointRec) * (size_t)J, hipMemcpyDeviceToHost);
    unsigned long long nj[4] = {0, 0, 0, 0}, cj[4] = {0, 0, 0, 0}, b3 = 0, b3lim = 0, c3lim = 0, f3 = 0, wh[5] = {0, 0, 0, 0, 0};
    for (auto &j : hj) if (j.kind == JK_DP) {
        const bool banded = (j.flags & 2u) != 0; const int q = j.qGap, r = j.rGap, ld = q > r ? q - r : r - q, W = banded ? 2 * ctx->P.bandWidth + ld + 1 : r + 1;
        const uint32_t cls = gapJointClass(gapJointKey(ctx->P, banded, q, r)); nj[cls]++; cj[cls] += (unsigned long long)q * (unsigned long long)std::min(W, r + 1);
        if (cls == 3) { if (banded) { b3++; if (W <= 32 && q <= YD_GROWS - 1 && r <= YD_GREF) { b3lim++; c3lim += (unsigned long long)q * W; } } else f3++;
            wh[std::min(4, (W - 17) / 8)]++; }
    }
    fprintf(stderr, "[ygpu] DP joints by class (band <= 12 / band <= 16 / other W <= 16 / the rest): %llu %llu %llu %llu; strip cells %llu %llu %llu %llu; "
                    "the rest: banded %llu (W <= 32 within the band kernels' limits: %llu, %llu cells), full %llu; "
                    "W 17-24 / 25-32 / 33-40 / 41-48 / more: %llu %llu %llu %llu %llu\n",
            nj[0], nj[1], nj[2], nj[3], cj[0], cj[1], cj[2], cj[3], b3, b3lim, c3lim, f3, wh[0], wh[1], wh[2], wh[3], wh[4]);
    // what phase 1's two passes see: the roots by fragments and by DP joints (k_p1_roots finishes those without one), the DP joints by the length of their op
    // list, the pure diagonals by length (the mask holds 64 bases)
    const uint32_t NC = ctx->nClumps; std::vector<uint32_t> jb((size_t)NC + 1); hipMemcpy(jb.data(), ctx->jointBase.p, 4ull * (NC + 1), hipMemcpyDeviceToHost);
    unsigned long long fr[6] = {0}, noDP = 0, noDPmulti = 0, oh[17] = {0}, dh[7] = {0}, nDiag = 0, nDPj = 0; const unsigned de[6] = {4, 8, 16, 32, 64, 128};
    for (uint32_t r = 0; r < NC; r++) {
        const uint32_t nj2 = jb[r + 1] - jb[r]; fr[std::min(5u, nj2)]++; bool dp = false;
        for (uint32_t k = jb[r]; k < jb[r + 1] && k < J; k++) dp |= hj[k].kind == JK_DP;
        noDP += !dp; noDPmulti += !dp && nj2 > 0;
    }
    for (auto &j : hj) { if (j.kind == JK_DP) { nDPj++; oh[j.nOps <= 15 ? j.nOps : 16]++; }
        if (j.kind == JK_DIAG) { nDiag++; int b = 0; while (b < 6 && j.qGap > de[b]) b++; dh[b]++; } }
    fprintf(stderr, "[ygpu] roots %u by fragments (1, 2, 3, 4, 5, more): %llu %llu %llu %llu %llu %llu; without a DP joint %llu (%.1f%%; %llu of them with joints)\n", NC,
            fr[0], fr[1], fr[2], fr[3], fr[4], fr[5], noDP, 100.0 * noDP / std::max(1u, NC), noDPmulti);
    fprintf(stderr, "[ygpu] DP joints %llu by ops (0 .. 15, more):", nDPj); for (int k = 0; k < 17; k++) fprintf(stderr, " %llu", oh[k]);
    fprintf(stderr, "; pure diagonals %llu by length (<= 4, 8, 16, 32, 64, 128, more):", nDiag); for (int k = 0; k < 7; k++) fprintf(stderr, " %llu", dh[k]); fprintf(stderr, "\n");
}

// YGPU_COUNT_DUPS: how many extension problems of the batch are exact duplicates (direction, strand, read, rOff, qOff, qLen)?
static void diagCountDups(ygpu_ctx *ctx, uint32_t nProb)
{
    std::vector<ExtProb> hp(nProb); hipMemcpy(hp.data(), ctx->extProbs.p, sizeof(ExtProb) * (size_t)nProb, hipMemcpyDeviceToHost);
    std::vector<std::array<uint32_t, 4>> keys; keys.reserve(nProb);
    for (auto &e : hp) if (e.flags & XP_VALID) keys.push_back({e.qBase, e.rOff, (uint32_t)e.qOff | ((uint32_t)e.qLen << 16), e.flags & 3u});
    std::sort(keys.begin(), keys.end()); size_t dup = 0, sameStart = 0;
    for (size_t k = 1; k < keys.size(); k++) { dup += keys[k] == keys[k - 1];
        sameStart += keys[k][0] == keys[k - 1][0] && keys[k][1] == keys[k - 1][1] && (keys[k][2] & 0xFFFF) == (keys[k - 1][2] & 0xFFFF) && keys[k][3] == keys[k - 1][3]; }
    fprintf(stderr, "[ygpu] extension problems: %zu valid, %zu exact duplicates (%.2f%%), %zu share (read, strand, direction, rOff, qOff) with their predecessor (%.2f%%)\n",
        keys.size(), dup, 100.0 * dup / std::max<size_t>(1, keys.size()), sameStart, 100.0 * sameStart / std::max<size_t>(1, keys.size()));
}

// YGPU_TRACE_LENS: the walks of the traceback, per problem and per wave of 64 in k_ext_rows' order
static void diagTraceLens(ygpu_ctx *ctx, const ExtArgs &E, uint32_t np)
{
    streamSync(ctx);
    std::vector<ExtRes> hr(np); std::vector<uint32_t> ho(np);
    hipMemcpy(hr.data(), E.res, sizeof(ExtRes) * (size_t)np, hipMemcpyDeviceToHost); hipMemcpy(ho.data(), E.order, 4ull * np, hipMemcpyDeviceToHost);
    unsigned long long walkers = 0, sumLen = 0, sumWaveMax = 0, sumRows = 0, hist[8] = {0};
    for (uint32_t w = 0; w < np; w += 64) { uint32_t mx = 0; for (uint32_t k = w; k < std::min(np, w + 64); k++) { const ExtRes &r = hr[ho[k]];
        const uint32_t len = r.score > 0 ? (uint32_t)r.maxi : 0u; walkers += r.score > 0; sumLen += len; sumRows += r.rows; mx = std::max(mx, len); int b = 0;
        while (b < 7 && (len >> (b + 3))) b++; hist[len ? b : 0] += 1; } sumWaveMax += mx; }
    fprintf(stderr, "[ygpu] traceback: %u problems, %llu walk (%.1f%%), mean walk %.1f rows (all) / %.1f (walkers), rows computed mean %.1f; sum over waves of "
        "the longest walk %llu = %.1f x the lanes' mean\n",
            np, walkers, 100.0 * walkers / np, (double)sumLen / np, (double)sumLen / std::max(1ull, walkers), (double)sumRows / np, sumWaveMax,
                (double)sumWaveMax * 64.0 / std::max(1ull, sumLen));
    fprintf(stderr, "[ygpu] walk length histogram (0..7, 8.., 16.., 32.., 64.., 128.., 256.., 512..):"); for (int b = 0; b < 8; b++) fprintf(stderr, " %llu", hist[b]);
        fprintf(stderr, "\n");
}

// YGPU_TRACE: the first access of k_ext_trace outside its strip, if there was one (gTraceDbg, ext_lanes.h)
static void diagTraceDbg(const ExtArgs &E)
{
    unsigned w8[8]; hipMemcpyFromSymbol(w8, HIP_SYMBOL(gTraceDbg), sizeof w8);
    if (!w8[0]) return;
    ExtRes rr; hipMemcpy(&rr, E.res + w8[6], sizeof rr, hipMemcpyDeviceToHost); ExtProb pp; hipMemcpy(&pp, E.probs + w8[6], sizeof pp, hipMemcpyDeviceToHost);
    fprintf(stderr, "[ygpu] k_ext_trace left its strip: dword %d of %u, f0 %u, laneOff %u; problem %u where %08x (wave %u lane %u phase %u) score %d maxi %d maxj "
        "%d rows %u qLen %u flags %u\n", (int)w8[1], w8[2], w8[3], w8[4], w8[6], w8[7], w8[7] >> 10, (w8[7] >> 4) & 63, w8[7] & 15, rr.score, rr.maxi, rr.maxj, rr.rows,
            pp.qLen, pp.flags);
    memset(w8, 0, sizeof w8); hipMemcpyToSymbol(HIP_SYMBOL(gTraceDbg), w8, sizeof w8);
}

// YGPU_TRACE: the roots k_split_lanes left to the wave kernel, and why (gFallWhy, split_lanes.h)
static void diagFallWhy(ygpu_ctx *ctx, const unsigned int *fallCount)
{
    uint32_t fc = 0; hipMemcpyAsync(&fc, fallCount, 4, hipMemcpyDeviceToHost, ctx->stream); streamSync(ctx);
    unsigned w8[8]; hipMemcpyFromSymbol(w8, HIP_SYMBOL(gFallWhy), sizeof w8);
    fprintf(stderr, "[ygpu] roots left to the wave kernel %u (other %u, DP not listed %u, second split %u, depth/list %u)\n", fc, w8[0], w8[1], w8[2], w8[3]);
    memset(w8, 0, sizeof w8); hipMemcpyToSymbol(HIP_SYMBOL(gFallWhy), w8, sizeof w8);
}

// YGPU_LIST_HIST: what k_p3_lanes walks -- the lengths of the three lists of a root (backward extension, phase-1 list, forward extension)
static void diagListHist(ygpu_ctx *ctx, uint32_t r0, uint32_t r1)
{
    const uint32_t nr2 = r1 - r0; std::vector<ExtRes> hr2(2 * (size_t)nr2); std::vector<RootState> hs(nr2);
    hipMemcpy(hr2.data(), ctx->extRes.as<ExtRes>() + 2 * (size_t)r0, sizeof(ExtRes) * hr2.size(), hipMemcpyDeviceToHost);
        hipMemcpy(hs.data(), ctx->rootState.as<RootState>() + r0, sizeof(RootState) * nr2, hipMemcpyDeviceToHost);
    unsigned long long hx[8] = {0}, hb[8] = {0}, ht[8] = {0}, sumx = 0, sumb = 0; const unsigned edges[7] = {0, 1, 2, 4, 8, 16, 32};
    auto bin = [&](unsigned v) { int k = 0; while (k < 7 && v > edges[k]) k++; return k; };
    for (uint32_t k = 0; k < nr2; k++) {
        const unsigned a = hr2[2 * k].score > 0 ? hr2[2 * k].nOps : 0u, c2 = hr2[2 * k + 1].score > 0 ? hr2[2 * k + 1].nOps : 0u, b = hs[k].len; hx[bin(a)]++;
        hx[bin(c2)]++; hb[bin(b)]++; ht[bin(a + b + c2)]++; sumx += a + c2; sumb += b; }
    fprintf(stderr, "[ygpu] list lengths over %u roots (bins: 0, 1, 2, 3-4, 5-8, 9-16, 17-32, more): extension lists", nr2);
        for (int k = 0; k < 8; k++) fprintf(stderr, " %llu", hx[k]);
    fprintf(stderr, "; phase-1 lists"); for (int k = 0; k < 8; k++) fprintf(stderr, " %llu", hb[k]); fprintf(stderr, "; merged");
        for (int k = 0; k < 8; k++) fprintf(stderr, " %llu", ht[k]);
    fprintf(stderr, "; mean ops per root: extensions %.1f, phase 1 %.1f\n", (double)sumx / nr2, (double)sumb / nr2);
}

// YD_PROF build: the in-kernel accounting of an attempt of the stage, zeroed before it and printed behind it
static void profReset()
{
#ifdef YD_PROF
    unsigned long long z[16] = {0}; hipMemcpyToSymbol(HIP_SYMBOL(gProf), z, sizeof z); hipMemcpyToSymbol(HIP_SYMBOL(gRowsProf), z, sizeof(unsigned long long) * 8);
    hipMemcpyToSymbol(HIP_SYMBOL(gTraceProf), z, sizeof(unsigned long long) * 8);
#endif
}
static void profPrint(ygpu_ctx *ctx, unsigned waves)
{
#ifdef YD_PROF
    streamSync(ctx); unsigned long long z[16]; hipMemcpyFromSymbol(z, HIP_SYMBOL(gProf), sizeof z);
    const char *nm[10] = {"root_total", "dp_rows", "traceback", "perfect_ext", "score", "emit", "split", "merge", "dp_calls", "roots"};
    fprintf(stderr, "[YD_PROF] waves %u:", waves); for (int i = 0; i < 10; i++) fprintf(stderr, " %s=%llu", nm[i], z[i]); fprintf(stderr, "\n");
    unsigned long long q[8]; hipMemcpyFromSymbol(q, HIP_SYMBOL(gRowsProf), sizeof q);      // k_ext_rows_pk: where its passes go
    if (q[0]) fprintf(stderr,
        "[YD_PROF] k_ext_rows_pk: wave passes %llu; of them writing results %.1f %%, with a new maximum in some lane %.1f %%, handing blocks over %.1f %%; "
            "refill rounds %.3f a pass (pool loads %.4f); busy lanes %.1f of 64\n",
                      q[0], 100.0 * q[1] / q[0], 100.0 * q[3] / q[0], 100.0 * q[5] / q[0], (double)q[2] / q[0], (double)q[6] / q[0], (double)q[4] / q[0]);
    unsigned long long t[8]; hipMemcpyFromSymbol(t, HIP_SYMBOL(gTraceProf), sizeof t);      // k_ext_trace_pk: where its passes go
    if (t[0]) fprintf(stderr, "[YD_PROF] k_ext_trace_pk: %llu waves that walk, %.1f passes a wave, %.1f active lanes a pass, %.2f rows a lane and pass; op groups %.2f a "
                              "lane-pass; lane-passes that end in a deletion run %.1f %%, in an insertion run %.1f %%\n",
                      t[0], (double)t[1] / t[0], (double)t[2] / t[1], (double)t[7] / t[2], (double)t[3] / t[2], 100.0 * t[5] / t[2], 100.0 * t[6] / t[2]);
#endif
}
