#!/usr/bin/env python3
"""What validating every removal of the rule-base reduction against K start states buys, on the CPU with the oracle (the model of
tests/reduce_starts_ref.py; DESIGN 4b-3's table).  Per demo: the rule base trained from the default start state; K validation starts =
the first K of spread_starts(64 candidates, seed 11) whose baseline episode is good; 200 independent test starts (seed 5) at the same
spread; per K in 1, 2, 4, 8, 16: (K, surviving rules, test starts the un-reduced rule base solves and the reduced one does not,
solved test starts that take more steps than before).  Takes about four minutes (cartpole's episodes run 1000 steps).
python tools/reduce_starts_table.py"""
import os, sys, time
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
from oracle import binding as ob
from tests import reduce_starts_ref as ref
from tests.test_hip_reduce_batch import Trained, spread_starts
from tests.test_reduce_starts_ref import default_agent
def run(env, spread, strategies):
    t,start=default_agent(env)
    probe=ob.Frirl(env,trig_mode=1)
    cand=spread_starts(probe,64,spread,11)
    probe=ob.Frirl(env,trig_mode=1)
    test=spread_starts(probe,200,spread,5)
    rp=ref.Replayer(t); allr=list(range(t.R0))
    good=[s for s in cand if rp.replay(allr,s)[1]>rp.good_above]
    base=[rp.replay(allr,s) for s in test]
    solved=[i for i,b in enumerate(base) if b[1]>rp.good_above]
    print(env,"rules",t.R0,"solved",len(solved),"of 200; good cands",len(good),flush=True)
    for st in strategies:
        row=[]
        for K in (1,2,4,8,16):
            o=ref.sequential(t,np.array(good[:K]),st)
            rp2=ref.Replayer(t)
            after=[rp2.replay(o.kept,test[i]) for i in solved]
            lost=sum(1 for a in after if not a[1]>rp.good_above)
            slower=sum(1 for i,a in zip(solved,after) if a[1]>rp.good_above and a[0]>base[i][0])
            row.append((K,len(o.kept),lost,slower))
        print(env,"strategy",st,row,flush=True)
t0=time.time()
run("mountaincar",0.3,(1,)); print(time.time()-t0)
run("cartpole",0.02,(1,)); print(time.time()-t0)
run("acrobot",0.05,(1,2)); print(time.time()-t0)
