#!/usr/bin/env python3
"""How many pixels every pair of raw Gear classes shares, and in which files (reference analyze_class_overlaps.py): the
analysis that justifies the priority rule spalling > pitting > scrape of csrc/polygon.hip, on the HIP path.

    python -m tiaozhanbei_unet_amd.analyze_gear_overlaps --data_root datasets/Gear [--splits train val test]

Same flags and defaults as the reference plus --batch_size (images per kernel launch) and --synthetic.  Per file only
the image header and the label text are read; ``augment.polygon_class_histogram`` counts the pixels of every set of raw
classes on the GPU and ``gear_overlaps.overlap_stats`` derives the report.  Writes
``<save_dir>/overlap_analysis_detailed.json`` in the reference's key layout (dict keys are strings, counts ints) plus a
``device_extras`` block; no PNG charts are drawn (gear_overlaps.py lists the differences).
"""
import argparse
import json
import os
import tempfile

FLAGS = [("--data_root", dict(type=str, default="datasets/Gear", help="Path to Gear dataset root directory")),
         ("--splits", dict(type=str, nargs="+", default=["train", "val", "test"], help="Dataset splits to analyze")),
         ("--save_dir", dict(type=str, default="overlap_analysis", help="Directory to save analysis results")),
         ("--batch_size", dict(type=int, default=32, help="Images per kernel launch")),
         ("--synthetic", dict(action="store_true", help="Analyze a small generated tree instead of --data_root"))]


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Analyze class overlaps in Gear dataset (MI355X HIP path)")
    for name, kw in FLAGS:
        p.add_argument(name, **kw)
    return p.parse_args(argv)


def print_report(stats):
    s = stats["summary"]
    print("\n" + "=" * 80 + "\nCLASS OVERLAP ANALYSIS RESULTS\n" + "=" * 80)
    print(f"Total files processed: {s['total_files_processed']}")
    print(f"Files with overlaps: {s['files_with_any_overlap']}")
    print(f"Percentage with overlaps: {s['percentage_files_with_overlap']:.2f}%")
    print("\nTotal pixels per class:")
    for name, pixels in s["total_pixels_per_class_name"].items():
        print(f"   {name:>10}: {pixels:>12,} pixels")
    print("\nOverlap Statistics:")
    print(f"{'Class Pair':<20} {'Overlap Pixels':<15} {'Files':<8} {'% of Class A':<12} {'% of Class B':<12}")
    print("-" * 80)
    for key, pixels in stats["overlap_pixels"].items():
        a, b = key.split("_vs_")
        pa = stats["overlap_percentages"].get(f"{key}_pct_of_{a}", 0)
        pb = stats["overlap_percentages"].get(f"{key}_pct_of_{b}", 0)
        print(f"{key:<20} {pixels:<15,} {len(stats['files_with_overlaps'][key]):<8} {pa:<11.2f}% {pb:<11.2f}%")
    if stats["detailed_stats"]:
        print("\nTop 10 largest overlaps:")
        print(f"{'File':<25} {'Classes':<20} {'Overlap':<10} {'Ratio A':<10} {'Ratio B':<10}")
        print("-" * 80)
        for d in sorted(stats["detailed_stats"], key=lambda x: x["overlap_pixels"], reverse=True)[:10]:
            print(f"{d['file'].split('/')[-1][:20]:<25} {d['class_a'] + ' vs ' + d['class_b']:<20} "
                  f"{d['overlap_pixels']:<10,} {d['overlap_ratio_a']:<9.3f} {d['overlap_ratio_b']:<9.3f}")
    x = stats["device_extras"]
    print(f"\nTriple overlap: {x['triple_overlap_pixels']:,} pixels")
    print("Pixels per class after priority resolution (spalling > pitting > scrape):")
    for name, pixels in x["pixels_per_class_after_priority"].items():
        print(f"   {name:>10}: {pixels:>12,} pixels")
    print("Polygon instances per class:")
    for name, k in x["polygon_instances_per_class"].items():
        print(f"   {name:>10}: {k:>12,}")


def print_recommendation(stats):
    pct = stats["summary"]["percentage_files_with_overlap"]
    print("\nRECOMMENDATIONS:\n" + "-" * 50)
    if pct > 10:
        print("HIGH OVERLAP DETECTED:\n   - priority-based resolution is STRONGLY recommended\n"
              "   - priority order: spalling > pitting > scrape")
    elif pct > 5:
        print("MODERATE OVERLAP DETECTED:\n   - priority-based resolution is recommended\n"
              "   - monitor training metrics for class imbalance")
    else:
        print("LOW OVERLAP DETECTED:\n   - priority-based resolution may still be beneficial")


def main(argv=None):
    import torch

    from . import gear_overlaps as GO
    args = parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("this build computes only on an AMD GPU (libunet_hip.so); there is no CPU path")
    if args.synthetic:
        from .gear_dataset import write_synthetic_gear
        args.data_root = write_synthetic_gear(tempfile.mkdtemp(prefix="gear_syn_"))
    print("Starting class overlap analysis...")
    print(f"Dataset root: {args.data_root}")
    print(f"Analyzing splits: {args.splits}")
    entries = GO.scan(args.data_root, args.splits)
    stats = GO.overlap_stats(GO.histograms(entries, args.batch_size))
    print_report(stats)
    os.makedirs(args.save_dir, exist_ok=True)
    path = os.path.join(args.save_dir, "overlap_analysis_detailed.json")
    with open(path, "w") as f:
        json.dump(GO.to_jsonable(stats), f, indent=2)
    print(f"\nDetailed results saved to: {path}")
    print_recommendation(stats)
    return stats


if __name__ == "__main__":
    main()
