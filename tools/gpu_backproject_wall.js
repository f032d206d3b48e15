'use strict';
/* node tools/gpu_backproject_wall.js [root] [calls] — wall time of camshift.Tracker.getBackProjectionImg() right after track(), from Node, at
 * 320x240 and 1920x1080: p50 / p90 over `calls` (default 40) track() + getBackProjectionImg() pairs after 5 warm-up pairs, and the p50 of the
 * track() next to it.  `root`: the checkout whose facade and addon are timed (default: this one) — run it in turn on a build of the parent
 * commit and on this one for an A/B in one GPU visit.  Says which route the facade took (the addon's camshiftBackProject wrapped and
 * counted here).  The frames: an orange ellipse that drifts over LCG noise.  Prints one JSON line per size. */
const path = require('path');
const root = path.resolve(process.argv[2] || path.join(__dirname, '..'));
const calls = +(process.argv[3] || 40);
const A = require(path.join(root, 'headtrackr_amd', 'js', 'headtrackr_hip.node'));
const headtrackr = require(path.join(root, 'headtrackr_amd', 'js', 'headtrackr.js'));
const { Canvas } = require(path.join(root, 'headtrackr_amd', 'js', 'canvas.js'));

let deviceCalls = 0;
if (typeof A.camshiftBackProject === 'function') {
  const real = A.camshiftBackProject;
  A.camshiftBackProject = function () { deviceCalls++; return real.apply(this, arguments); };
}
const now = function () { return Number(process.hrtime.bigint()) / 1e6; };
const pct = function (v, q) { const s = v.slice().sort(function (a, b) { return a - b; }); return +s[Math.min(s.length - 1, Math.floor(q / 100 * s.length))].toFixed(3); };

function frame(w, h, cx, cy, a, b, seed) {
  const px = new Uint8Array(w * h * 4);
  let s = seed >>> 0;
  for (let y = 0; y < h; y++) {
    for (let x = 0; x < w; x++) {
      const p = (y * w + x) * 4, dx = (x - cx) / a, dy = (y - cy) / b;
      s = (Math.imul(s, 1664525) + 1013904223) >>> 0;
      if (dx * dx + dy * dy <= 1) { px[p] = 200 + (s >>> 28); px[p + 1] = 60 + (s >>> 28); px[p + 2] = 40; } else { px[p] = s >>> 24; px[p + 1] = (s >>> 16) & 255; px[p + 2] = (s >>> 8) & 255; }
      px[p + 3] = 255;
    }
  }
  return px;
}

[[320, 240], [1920, 1080]].forEach(function (sz) {
  const w = sz[0], h = sz[1], a = w >> 3, b = h >> 3, nf = 4;
  const canvases = [];
  for (let k = 0; k < nf; k++) canvases.push(new Canvas(w, h).setFrame(frame(w, h, (w >> 1) + 2 * k, (h >> 1) + k, a, b, 77 + k)));
  const tracker = new headtrackr.camshift.Tracker({ calcAngles: true });
  tracker.initTracker(canvases[0], new headtrackr.camshift.Rectangle((w >> 1) - a, (h >> 1) - b, 2 * a, 2 * b));
  const tTrack = [], tBp = [];
  const before = deviceCalls;
  let sum = 0;
  for (let i = 0; i < calls + 5; i++) {
    const t0 = now();
    tracker.track(canvases[1 + i % (nf - 1)]);
    const t1 = now();
    const img = tracker.getBackProjectionImg();
    const t2 = now();
    sum += img.data[(h >> 1) * w * 4 + (w >> 1) * 4];
    if (i >= 5) { tTrack.push(t1 - t0); tBp.push(t2 - t1); }
  }
  tracker.release();
  console.log(JSON.stringify({ root: root, size: w + 'x' + h, calls: calls, route: deviceCalls > before ? 'device' : 'host',
    getBackProjectionImg_ms_p50: pct(tBp, 50), getBackProjectionImg_ms_p90: pct(tBp, 90), track_ms_p50: pct(tTrack, 50), centre_value_sum: sum }));
});
process.stdout.write('', function () { headtrackr.exitNow(0); });
