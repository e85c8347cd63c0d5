#!/usr/bin/env python3
"""Which hardware queue every stream of a streaming run dispatched to: from a rocprofv3 --kernel-trace results .db (or a *_kernel_trace.csv),
one line per stream with the stage its kernels belong to, its queue and its dispatch count, then the streams that share a queue.  Two stages on
one queue run in single file: a barrier packet (hipStreamWaitEvent on an event that has not fired yet) at the head of the queue holds back
every packet behind it, whichever stream enqueued it.   python tools/queue_map.py <rocprof output dir>"""
import collections
import csv
import glob
import sqlite3
import sys

STAGE_KERNELS = [('sr', 'k_sr_first_last'), ('ds', 'k_map_ds_bin'), ('lo', 'k_lo_assoc'), ('map', 'k_map_prepare'), ('img', 'k_img_'),
                 ('vo', 'k_vo_')]


def short(n):
    return n.split('(')[0].replace('vloam::', '').replace('void ', '').split('<')[0]


def load(root):
    dbs = glob.glob(root + '/**/*.db', recursive=True)
    if dbs:
        c = sqlite3.connect(dbs[0])
        tabs = [r[0] for r in c.execute("select name from sqlite_master where type in ('table','view')")]
        kt = [t for t in tabs if t.startswith('kernels')][0]
        cols = [r[1] for r in c.execute('pragma table_info(%s)' % kt)]
        qcol = [x for x in cols if x.lower() in ('queue_id', 'queue')][0]
        return c.execute('select name, stream_id, %s, start from %s order by start' % (qcol, kt)).fetchall()
    rows = []
    for f in glob.glob(root + '/**/*kernel_trace.csv', recursive=True):
        for r in csv.DictReader(open(f)):
            rows.append((r['Kernel_Name'], int(r['Stream_Id']), int(r['Queue_Id']), int(r['Start_Timestamp'])))
    return sorted(rows, key=lambda r: r[3])


rows = load(sys.argv[1])
streams = collections.OrderedDict()   # stream -> [queues, kernel names, dispatches, first dispatch]
for name, st, q, t in rows:
    e = streams.setdefault(st, [set(), set(), 0, t])
    e[0].add(q)
    e[1].add(short(name))
    e[2] += 1


def stage_of(names):
    found = [s for s, k in STAGE_KERNELS if any(n.startswith(k) for n in names)]
    if 'lo' in found and 'k_sr_ring' in names:   # the SR stream also launches odometry-side grid builds, never k_lo_assoc; keep it 'sr'
        found.remove('lo')
    return '+'.join(found) or ','.join(sorted(names))[:60]


t0 = rows[0][3] if rows else 0
print('%-8s %-12s %-10s %10s  %s' % ('stream', 'stage', 'queue', 'dispatches', 'first dispatch (ms from the first)'))
by_q = collections.defaultdict(list)
for st, (qs, names, nd, t) in streams.items():
    stg = stage_of(names)
    print('%-8s %-12s %-10s %10d  %.3f' % (st, stg, ','.join(str(q) for q in sorted(qs)), nd, (t - t0) / 1e6))
    for q in qs:
        by_q[q].append(stg)
print('queues: %d distinct; shared: %s' % (len(by_q), '; '.join('q%s <- %s' % (q, ' + '.join(v)) for q, v in by_q.items() if len(v) > 1) or 'none'))
