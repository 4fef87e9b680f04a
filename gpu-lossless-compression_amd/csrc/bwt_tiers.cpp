// bwt_tiers.cpp -- the suffix sorter's host side: which tier's output is final for a block.  A call goes down a ladder:
//   bucket sorter (bwt_bucket.hip) -> sample sorter, first and second attempt (bwt_sample.hip) -> periodic tier
//   (bwt_periodic.hip) -> resumed doubling (tolerant sample sort + bwt_sa.hip's doubling rounds) -> general sorter (bwt_sa.hip).
// Every tier takes the blocks the ones before it gave up on, `left` of them, and leaves the count of what it gives up on
// in turn; the host learns each count by one readback (sa_read), a ~5 us link in the chain a single call waits for.  No
// kernels here: the tiers' launchers are in the files named above.
#include "glc_internal.h"

namespace glc {

// Two-phase form, so that a caller can queue the stages that FOLLOW the sort before the host waits for the sorter's
// one readback (cudpp_api.cpp queues MTF + Huffman speculatively: the GPU never idles behind the wait, and the
// rare batch with flagged blocks re-runs them):
//   sa_build_begin   enqueues the bucket sorter and the readback of the flagged-block count (an event marks it);
//                    with s.sorter 1 or 2 it runs the whole general sort instead (which blocks per round).
//   sa_build_finish  waits for that event only; if blocks were flagged, enqueues the other tiers for them.
//                    *nflagged > 0 tells the caller that bwt_out / d_index of those blocks were rewritten.
hipError_t sa_build_begin(const SortCall &c, SaScratch &s)
{
    if (c.n == 0 || c.n > s.nmax || c.n > MAX_BLOCK_ELEMS || c.nblk == 0 || c.nblk > s.rows) return hipErrorInvalidValue;
    s.stats = SortStats();
    s.stats.flagged = s.stats.general = c.nblk;
    s.pending = false;
    if (s.sorter == 1 || s.sorter == 2) {
        const bool isa = s.force_isa;
        s.force_isa = isa || s.sorter == 2;
        const hipError_t e = sa_build_general(c, s, nullptr, c.nblk);
        s.force_isa = isa;
        return e;
    }
    // bucket sorter first; the suffix array itself is only written when it is the result asked for
    if (!c.bwt_out) GLC_TRY(sa_general_reserve(s, true));
    s.skip_tier1 = sa_skips_tier1(s, c.nblk);                // the caller knows its data is text-like (sorter 4), or the plan's last calls say so
    GLC_TRY(fs_build(c, s));
    // (the flagged-block count is in s.h_max_cnt[HW_FLAGGED] when the pass's last kernel is through: it writes it there itself
    //  -- k_fs_finish -- where a copy command behind the pass was one more ~5 us link in a single call's chain)
    if (!s.ev_flag) GLC_TRY(hipEventCreateWithFlags(&s.ev_flag, hipEventDisableTiming));
    GLC_TRY(hipEventRecord(s.ev_flag, c.st));
    s.pending = true;
    return hipSuccess;
}

// The tiers.  Each takes the call, the scratch and `left`, the number of blocks every tier so far gave up on (they keep n in
// s.fs_lcnt), queues its work for them and leaves in `left` what it gives up on too.  The blocks the bucket sorter flagged,
// s.stats.flagged of them, stay listed in s.ss_list throughout.

// second tier: string sample sort of the flagged blocks; what it gives up on (very deep repeats) is counted again
static hipError_t tier_sample(const SortCall &c, SaScratch &s, uint32_t &left)
{
    const uint32_t *w;
    GLC_TRY(ss_build(c, s, left));
    GLC_TRY(sa_read(c.st, s, w, HW_GIVEN_UP, s.fs_nflag + 1));
    left = w[0];
    return hipSuccess;
}

// some blocks were given up on.  Those whose only trouble was a bucket past its slot get ONE more attempt with
// other samples (a bucket of 4033-4200 words where 4032 fit: ~1 % of log-style blocks; the general sorter
// costs ten times the sample sorter, and its rounds hold the host)
static hipError_t tier_sample_again(const SortCall &c, SaScratch &s, uint32_t &left)
{
    if (!left) return hipSuccess;
    const uint32_t nflag = s.stats.flagged, *w;
    if (s.stage_partial) GLC_TRY(ss_split_masks(c.st, c.nblk, s));
    GLC_TRY(ss_retry_prepare(c.st, nflag, s));
    GLC_TRY(sa_read(c.st, s, w, HW_LISTED, s.fs_nflag + 2));
    const uint32_t again = w[0];
    s.stats.retried += again;
    if (!again) return hipSuccess;
    if (s.stage_partial && left < nflag) {
        // the stages behind the sort for the blocks the first attempt finished, on a side stream BESIDE the second attempt
        // (ss_mask was written before ss_retry_prepare touched anything: see above)
        // (each of the three is made where it is missing: a call that failed between them leaves the next one the rest to
        //  make, not a stream without its events)
        if (!s.aux) {
            // (lowest priority: the side stream's kernels fill the chip, the second attempt's small launches on `st` are a
            //  chain of latencies -- with equal priorities its bucketing pass took 614 us beside k_mtf_encode instead of 27)
            int least = 0, greatest = 0;
            (void)hipDeviceGetStreamPriorityRange(&least, &greatest);
            GLC_TRY(hipStreamCreateWithPriority(&s.aux, hipStreamNonBlocking, least));
        }
        if (!s.ev_fork) GLC_TRY(hipEventCreateWithFlags(&s.ev_fork, hipEventDisableTiming));
        if (!s.ev_join) GLC_TRY(hipEventCreateWithFlags(&s.ev_join, hipEventDisableTiming));
        GLC_TRY(hipEventRecord(s.ev_fork, c.st));
        GLC_TRY(hipStreamWaitEvent(s.aux, s.ev_fork, 0));
        GLC_TRY(s.stage_partial(s.aux, s.ss_mask[0]));
        GLC_TRY(hipEventRecord(s.ev_join, s.aux));
        s.partial_used = true;
    }
    GLC_TRY(sa_set_left(c.st, s, left - again));               // the others stay given up on; the second attempt adds its own
    GLC_TRY(ss_build(c, s, again, 1));
    GLC_TRY(sa_read(c.st, s, w, HW_GIVEN_UP, s.fs_nflag + 1));
    left = w[0];
    return hipSuccess;
}

// Blocks that are ONE periodic stretch (a page repeated, a short pattern, one byte up to a different last one):
// every suffix ties with the one a period further on for nearly the whole block -- ~18 doubling rounds over a
// million live suffixes.  Their suffix array has a closed form over the sorted rotations of the period and the
// few suffixes around the break (bwt_periodic.hip); only those -- a text of <= 7 p + 2 bytes per block -- are
// sorted, by the general sorter, whatever the block's size.
static hipError_t tier_periodic(const SortCall &c, SaScratch &s, uint32_t &left)
{
    if (!left || !s.periodic || !c.bwt_out || !c.d_index || c.n < 16 * PER_PMAX || s.nmax < PER_NU) return hipSuccess;
    const uint32_t *w;
    GLC_TRY(per_reserve(s));
    GLC_TRY(per_detect(c, s, s.stats.flagged));
    GLC_TRY(sa_read(c.st, s, w, HW_PER_TAKEN, s.per_count, 2));   // with HW_PER_LONGEST
    const uint32_t nper = w[0] < PER_TAKE ? w[0] : PER_TAKE;   // (k_per_detect takes no more than its scratch holds)
    if (!nper) return hipSuccess;
    // (the longest text of representatives among the taken blocks -- they are sorted as one batch of equal length -- comes
    //  with the count: round 5 copied every block's info to the host and waited a second time for it: ADVICE r5)
    uint32_t nu = w[1] < 64 ? 64 : w[1];
    nu = (nu + 15u) & ~15u;
    if (nu > PER_NU) nu = PER_NU;
    GLC_TRY(per_text(c, s, nper, nu));
    GLC_TRY(sa_build_general(SortCall{c.st, s.per_text, PER_NU, nu, nper, nullptr, 0, nullptr}, s, nullptr, nper));
    GLC_TRY(per_expand(c, s, nper, nu));
    GLC_TRY(sa_read(c.st, s, w, HW_PER_DONE, s.per_count + 2));
    const uint32_t done = w[0];
    s.stats.periodic += done;
    left -= done < left ? done : left;
    return sa_set_left(c.st, s, left);                         // the device-side count of blocks still given up on follows
}

// Blocks whose only trouble was a repeat deeper than the cap (zero pages, a duplicated region, long periodic
// stretches inside otherwise ordinary data): the sample sorter once more, in its TOLERANT form and writing the
// suffix array -- everything it can order it orders, suffixes that agree in more than the cap stay as they come
// -- then prefix doubling from that depth on, over the groups of rows that still share the cap (a few thousand
// suffixes of such a block for ~11 rounds, where the general sorter from scratch takes a million through ~20).
static hipError_t tier_resume(const SortCall &c, SaScratch &s, uint32_t &left)
{
    if (!left || !s.resume_min) return hipSuccess;
    const uint32_t nflag = s.stats.flagged, *w;
    // counted first, without touching anything: below resume_min the blocks go on as they are (their flags and fills
    // stay what glcPlanDebugSortFlags / BucketFill report)
    GLC_TRY(ss_retry_prepare(c.st, nflag, s, 2, true));
    GLC_TRY(sa_read(c.st, s, w, HW_LISTED, s.fs_nflag + 2));
    const uint32_t deep2 = w[0];
    // (a few blocks: the extra pass and its launches cost what the shorter doubling saves -- 2.6 against 2.2-2.7 ms for
    //  one block, 3.5 against 4.4 for eight)
    if (deep2 < s.resume_min) return hipSuccess;
    GLC_TRY(ss_retry_prepare(c.st, nflag, s, 2));              // listed, flags and fills cleared for the tolerant pass
    GLC_TRY(sa_general_reserve(s, false));
    GLC_TRY(sa_set_left(c.st, s, left - deep2));               // the others stay given up on; this attempt adds its own
    SortCall rows = c;                                         // the tolerant form writes suffix-array rows, no BWT
    rows.bwt_out = nullptr; rows.bwt_stride = 0; rows.d_index = nullptr;
    GLC_TRY(ss_build(rows, s, deep2, 2));
    GLC_TRY(sa_read_queue(c.st, s, HW_GIVEN_UP, s.fs_nflag + 1));   // (one wait for the count and for the words behind it)
    GLC_TRY(grp_keys(c, s, deep2));
    GLC_TRY(sa_read_wait(c.st, s));
    const uint32_t left2 = s.h_max_cnt[HW_GIVEN_UP];           // = left - deep2 + what the tolerant form gave up on (a bucket past its slot)
    const uint32_t resumed = left - left2;
    if (resumed) GLC_TRY(sa_build_general(c, s, s.ss_cnt2, resumed, SS_TOL_CAP));
    s.stats.resumed += resumed;
    left = left2;
    return hipSuccess;
}

// whatever is left: the general sorter from the text
static hipError_t tier_general(const SortCall &c, SaScratch &s, uint32_t &left)
{
    return left ? sa_build_general(c, s, s.fs_lcnt, left) : hipSuccess;
}

static hipError_t sa_build_tiers(const SortCall &c, SaScratch &s, uint32_t *nflagged)
{
    if (nflagged) *nflagged = 0;
    if (!s.pending) return hipSuccess;                       // general sorter only: nothing was deferred
    s.pending = false;
    GLC_TRY(hipEventSynchronize(s.ev_flag));
    const uint32_t nflag = s.h_max_cnt[HW_FLAGGED];
    // the streak of calls whose every block the probe called text-like (k_fs_finish counts the others, in skipped calls too)
    s.textlike_streak = (nflag == c.nblk && s.h_max_cnt[HW_NOT_TEXTLIKE] == 0) ? (s.textlike_streak < 1000u ? s.textlike_streak + 1 : 1000u) : 0u;
    s.stats.skipped = s.skip_tier1;
    s.stats.flagged = nflag;                                   // the bucket sorter's attempt is through: what it left, ...
    s.stats.general = 0;                                       // ... of which the sample sorter's share is not known yet
    if (nflag == 0) return hipSuccess;
    if (nflagged) *nflagged = nflag;
    uint32_t left = nflag;
    if (s.sorter == 3) s.stats.general += left;                // no sample sorter, and none of the tiers that start from its flags
    else {
        GLC_TRY(tier_sample(c, s, left));
        GLC_TRY(tier_sample_again(c, s, left));
        s.stats.general += left;                               // what the sample sorter (both attempts) gave up on
        GLC_TRY(tier_periodic(c, s, left));
        GLC_TRY(tier_resume(c, s, left));
    }
    return tier_general(c, s, left);
}

hipError_t sa_build_finish(const SortCall &c, SaScratch &s, uint32_t *nflagged)
{
    s.partial_used = false;
    const hipError_t e = sa_build_tiers(c, s, nflagged);
    // whatever the tiers did, the side stream's stages (if any were queued) are joined into st here
    if (s.partial_used) { const hipError_t j = hipStreamWaitEvent(c.st, s.ev_join, 0); if (e == hipSuccess && j != hipSuccess) return j; }
    return e;
}

hipError_t sa_build(const SortCall &c, SaScratch &s)
{
    GLC_TRY(sa_build_begin(c, s));
    return sa_build_finish(c, s, nullptr);
}

} // namespace glc
