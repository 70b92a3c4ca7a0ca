"""Per-XCD dealing of an ordered batch's tickets (csrc/device_tickets.h), on the host: the header's own mapping and claim loop compiled
with a stub runtime.  Ticket k of counter x -> position ((k / C) * 8 + x) * C + k % C is a bijection onto [0, n), and waves that claim
through xcd_ticket_claim from any mix of counters (stealing when theirs runs out) take every position exactly once, then all stop."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pg_embedding_amd", "csrc")

STUB = r"""
#pragma once
#include <stdint.h>
#include <stddef.h>
#define __host__
#define __device__
#define __forceinline__ inline
#define __builtin_amdgcn_readfirstlane(v) (v)
static unsigned g_xcc;                       // the XCC id the next claim's wave runs on
#define __builtin_amdgcn_s_getreg(v) g_xcc
static inline uint32_t atomicAdd(uint32_t *p, uint32_t v) { uint32_t o = *p; *p = o + v; return o; }
"""

MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "device_tickets.h"
using namespace pgemb;

// mapping: every (counter, ticket) below the end lands on a distinct position in [0, n), and every position is hit
static int bijection(uint32_t n, uint32_t log2c)
{
	std::vector<int> hit(n, 0);
	const uint32_t c = 1u << log2c;
	for (uint32_t x = 0; x < XCD_TICKETS; x++)
		for (uint32_t k = 0; k < n + 2 * c; k++)
		{
			const uint32_t p = xcd_ticket_position(k, x, log2c);
			if (p < n) hit[p]++;
			if (k > 0 && p <= xcd_ticket_position(k - 1, x, log2c)) return 1;     // grows with k: exhausted stays exhausted
		}
	for (uint32_t i = 0; i < n; i++) if (hit[i] != 1) return 2;
	return 0;
}

// claims: `waves` waves on counters given by `home` (-1: wave % 8) take positions in a pseudo-random interleaving until all stop
static int claims(uint32_t n, uint32_t log2c, uint32_t waves, int home, uint32_t seed)
{
	uint32_t counters[XCD_TICKETS * XCD_TICKET_WORDS] = {};
	std::vector<bool> done(waves, false);
	std::vector<int> hit(n, 0);
	uint32_t live = waves, r = seed * 2654435761u + 1;
	while (live)
	{
		r = r * 1664525u + 1013904223u;
		const uint32_t w = (r >> 8) % waves;
		if (done[w]) continue;
		g_xcc = home >= 0 ? (uint32_t) home : w % XCD_TICKETS;
		const uint32_t p = xcd_ticket_claim(counters, n, log2c, 0);
		if (p >= n) { done[w] = true; live--; continue; }
		hit[p]++;
	}
	for (uint32_t i = 0; i < n; i++) if (hit[i] != 1) return 3;
	return 0;
}

int main()
{
	const uint32_t ns[] = { 1, 7, 63, 64, 100, 511, 512, 513, 4095, 8192, 8193, 40000 };
	int bad = 0;
	for (uint32_t n : ns)
		for (uint32_t lc = 1; lc <= 9; lc++)
		{
			if (int e = bijection(n, lc)) { printf("bijection n=%u C=%u: %d\n", n, 1u << lc, e); bad++; }
			if (n <= 8193)
			for (int home : { -1, 0, 5 })
				for (uint32_t waves : { 1u, 3u, 9u, 64u })
					if (int e = claims(n, lc, waves, home, n + lc + waves)) { printf("claims n=%u C=%u waves=%u home=%d: %d\n", n, 1u << lc, waves, home, e); bad++; }
		}
	printf("%s\n", bad ? "FAIL" : "OK");
	return bad ? 1 : 0;
}
"""


def _cxx():
    for c in ("/opt/rocm/lib/llvm/bin/clang++", shutil.which("clang++"), shutil.which("g++")):
        if c and os.path.exists(c):
            return c
    pytest.skip("no host C++ compiler")


def test_ticket_mapping_is_a_bijection_and_claims_cover_every_position_once(tmp_path):
    os.makedirs(tmp_path / "hip")
    (tmp_path / "hip" / "hip_runtime.h").write_text(STUB)
    (tmp_path / "main.cpp").write_text(MAIN)
    exe = str(tmp_path / "t")
    subprocess.run([_cxx(), "-std=c++17", "-O2", "-I", str(tmp_path), "-I", CSRC, str(tmp_path / "main.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout[-3000:]
