"""rocprofv3 kernel trace (csv) -> the compact csv.gz that tools/trace_streams.py and tools/trace_region.py read
(name,queue,stream,start,end,wg,grid; kernel names cut to 60 characters):

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o k -- python bench.py --no-cpu-baseline
    python tools/trace_compact.py DIR/k_kernel_trace.csv trace_compact.csv.gz"""
import csv
import gzip
import sys

src, dst = sys.argv[1], sys.argv[2]
with open(src, newline="") as f, gzip.open(dst, "wt") as g:
    g.write("name,queue,stream,start,end,wg,grid\n")
    for r in csv.DictReader(f):
        name = r["Kernel_Name"][:60].replace("\n", " ")
        g.write(f'{name},{r["Queue_Id"]},{r["Stream_Id"]},{r["Start_Timestamp"]},{r["End_Timestamp"]},'
                f'{r["Workgroup_Size_X"]},{r["Grid_Size_X"]}\n')
