#!/usr/bin/env python3
"""Has a change of the source changed any kernel's instructions?  Two outputs of
  hipcc --offload-arch=gfx950 -O3 -std=c++17 -Iinclude -Ihutoken_amd/csrc --cuda-device-only -S -o X.s hutoken_amd/csrc/FILE.hip
(both compiled from the same relative path, or their .file lines differ) compared function by function:
  python tools/isa_funcs.py before.s after.s   ->   same / DIFF, both line counts, the demangled name."""
import sys,re,hashlib,subprocess
def funcs(path):
    out={};cur=None;buf=[]
    for line in open(path):
        m=re.match(r'^(_Z\w+|\w+):\s*; @',line)
        if m: cur=m.group(1);buf=[]
        if cur is not None:  # (labels carry the function's ordinal: in the code, in loop comments, and in the comments' column)
            buf.append(re.sub(r'\s+',' ',re.sub(r'\bBB\d+_','BB_',re.sub(r'\.L(BB|func_end|func_begin|JTI)\d+','.L\\1',line)))+'\n')
        if cur and line.startswith('.Lfunc_end'):
            out[cur]=(hashlib.sha256(''.join(buf).encode()).hexdigest()[:12],len(buf));cur=None
    return out
a,b=funcs(sys.argv[1]),funcs(sys.argv[2])
names=sorted(set(a)|set(b))
dem=subprocess.run(['c++filt']+names,capture_output=True,text=True).stdout.split('\n')
for n,d in zip(names,dem):
    s='same' if a.get(n)==b.get(n) else 'DIFF'
    print(s,a.get(n,('-',0))[1],b.get(n,('-',0))[1],d[:150])
