"""Time of the Gibbs recursion on a finished tape (2000 iterations) by model size, in one piece and in verified segments
(fokl_gibbs_chain_segments_host: pieces across SIMD lanes, and FOKL_HCHAIN_MAPPING=pieces, one after the other);
FOKL_CHAIN_ISA=base|avx2|avx512 picks the vector statement (development aid)."""
import sys, time, numpy as np
import os
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from fokl_gpy_amd import _capi


def best_of(fn, args, repeats=20):
    best = 1e9
    for r in range(repeats):
        t = time.perf_counter(); out = fn(*args); best = min(best, time.perf_counter() - t)
    return best, out


np.random.seed(5)
print('p1  serial us (ns/iter)  lanes us  pieces us  bad_cut  max |w - w_serial| / column scale  w[-1,0]  sum(w)')
for p1 in (20, 60, 100, 144):
    s=_capi.LegacyStream()
    tape=_capi.noise_tape(p1, 2000, 5e5+p1/2, 3+p1/2, s)
    _capi.finish_tape_blocks(tape)
    lamb=np.sort(np.random.rand(p1)*1e5+10); qty=np.random.randn(p1)*100
    args=(lamb,qty,900.0,2.0,5e5,0.3,0.9,tape)
    best,(w,f)=best_of(_capi.gibbs_chain_from_finished_tape, args)
    os.environ['FOKL_HCHAIN_MAPPING']='lanes'
    lanes,(wl,fl,bad)=best_of(_capi.gibbs_chain_segments_host, args)
    os.environ['FOKL_HCHAIN_MAPPING']='pieces'
    pieces,(wp,fp,badp)=best_of(_capi.gibbs_chain_segments_host, args)
    del os.environ['FOKL_HCHAIN_MAPPING']
    assert np.array_equal(wl, wp) and f == fl == fp
    print(p1, round(best*1e6,1),'us', round(best/2000*1e9,1),'ns/iter', round(lanes*1e6,1), round(pieces*1e6,1), int(bad),
          float((np.abs(wl-w)/np.abs(w).max(0)).max()), float(w[-1,0]), float(w.sum()))
