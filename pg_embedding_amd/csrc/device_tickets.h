// device_tickets.h — per-XCD dealing of an ordered batch's tickets.
//
// A batch in locality order (device_order.h) has the queries of one region of the table next to each other.  With one global ticket
// the blocks that take them are dealt round-robin over the 8 XCDs, so a region's ~40 walks land on all eight L2s and each L2 sees 1/8 of
// that region's reuse.  Here the ordered batch is cut into chunks of C positions and the chunks are dealt round-robin over 8 counters:
// counter x owns chunks x, x + 8, x + 16, ...  A wave claims from the counter of the XCD it runs on, so every XCD moves along the same
// front of the order and a region's chunk stays on one XCD, whose L2 then serves the rows its walks share.
//
//   ticket k of counter x  ->  position ((k / C) * 8 + x) * C + k % C of the ordered batch (positions >= n are skipped)
//
// Every position below n belongs to exactly one (counter, ticket).  Positions grow with k, so a counter that has handed out a
// position >= n is exhausted for good.  A wave whose counter is exhausted moves on to x + 1, x + 2, ... (mod 8) and claims there; it
// stops when all eight are exhausted, so no wave idles while any query is left.  Placement is for
// speed only: any wave may claim from any counter, and which wave walks which query never changes a result.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pgemb {

constexpr uint32_t XCD_TICKETS = 8;                  // counters (the XCDs of an MI355X)
constexpr uint32_t XCD_TICKET_WORDS = 32;            // one counter per 128-byte line
constexpr size_t XCD_TICKET_BYTES = XCD_TICKETS * XCD_TICKET_WORDS * 4;

// position of ticket k of counter x at chunk size C (a power of two, 1 << log2c).  32-bit: the host deals only batches of fewer than
// XCD_TICKETS_MAX_NQ queries, so a counter's tickets, its end and every wave's one look past it included, stay far below 2^28 and
// their positions below 2^31.
constexpr uint32_t XCD_TICKETS_MAX_NQ = 1u << 26;
__host__ __device__ __forceinline__ uint32_t xcd_ticket_position(uint32_t k, uint32_t x, uint32_t log2c)
{
	return ((((k >> log2c) * XCD_TICKETS) + x) << log2c) + (k & ((1u << log2c) - 1u));
}

#ifdef PGEMB_SIMT_EMULATOR
// (the emulator has no XCDs: blocks are dealt as the dispatcher deals them, blockIdx.x % 8; PGEMB_EMU_XCD_ID=i puts every wave on
// counter i, so that stealing has to carry the whole batch)
__device__ __forceinline__ uint32_t xcd_id()
{
	static const int forced = [] { const char *s = getenv("PGEMB_EMU_XCD_ID"); return s && *s ? atoi(s) : -1; }();
	return forced >= 0 ? (uint32_t) forced % XCD_TICKETS : (uint32_t) blockIdx.x % XCD_TICKETS;
}
#else
// the XCD this wave runs on: s_getreg_b32 of HW_REG_XCC_ID (hwreg 20, bits 0..3)
__device__ __forceinline__ uint32_t xcd_id() { return (uint32_t) __builtin_amdgcn_s_getreg((3 << 11) | 20) % XCD_TICKETS; }
#endif

// The next position of the ordered batch for this wave (wave-uniform), or n when every counter is exhausted.  counters: XCD_TICKETS
// words XCD_TICKET_WORDS apart, zeroed before the launch.  The wave starts at the counter of its own XCD and moves on to x + 1, x + 2, ...
// while they are exhausted.  It keeps no state between claims (a live register across the walk costs the search kernels registers
// they do not have): once its own counter is exhausted, each later claim of the wave pays one more atomic per exhausted counter it
// passes, at most 7, and only in the last ~1/16 of a launch, where the counters run out.
__device__ __forceinline__ uint32_t xcd_ticket_claim(uint32_t *counters, uint32_t n, uint32_t log2c, uint32_t lane)
{
	uint32_t x = xcd_id();
#pragma unroll 1                                     // (unrolled, the eight tries cost the widest beam kernels SGPRs)
	for (uint32_t tries = 0; tries < XCD_TICKETS; tries++)
	{
		uint32_t k = 0;
		if (lane == 0) k = atomicAdd(counters + x * XCD_TICKET_WORDS, 1u);
		k = __builtin_amdgcn_readfirstlane(k);
		const uint32_t pos = xcd_ticket_position(k, x, log2c);
		if (pos < n) return pos;
		x = (x + 1) % XCD_TICKETS;
	}
	return n;
}

}  // namespace pgemb
