'use strict';
/* node tools/gpu_ingest_wall.js [root] [steps] — wall time of headtrackr.Tracker.step() from Node with a video larger than the 320x240 work
 * canvas (640x480, 1280x720, 1920x1080), the step's drawImage (main.js:170) on the host (canvas.js's loop) against the device route
 * (ccv.drawFrames: upload of the video frame, ht_draw_frames_device, download of the canvas).  The route is forced from here, whatever
 * step() itself would choose: for the device route the work canvas's own drawImage is replaced by one that calls ccv.drawFrames, for the
 * host route ccv.drawFrames is replaced by the canvas's loop.  Three rounds of (one warm-up block + one timed block of `steps`, default
 * 30, steps) per route, the routes alternating; p50 per route.  Also the two draws alone, outside the loop.  `root`: the checkout whose
 * facade and addon are timed (default: this one); a build of the parent commit has no device route and reports the host numbers only.  The frames: a vote-image-like bright square drifting over a flat background (the tracker goes VJ -> CS or stays in VJ;
 * either way every step draws).  Prints one JSON line per size. */
const path = require('path');
const root = path.resolve(process.argv[2] || path.join(__dirname, '..'));
const steps = +(process.argv[3] || 30);
const headtrackr = require(path.join(root, 'headtrackr_amd', 'js', 'headtrackr.js'));
const { Canvas } = require(path.join(root, 'headtrackr_amd', 'js', 'canvas.js'));

const now = function () { return Number(process.hrtime.bigint()) / 1e6; };
const p50 = function (v) { const s = v.slice().sort(function (a, b) { return a - b; }); return +s[Math.floor(s.length / 2)].toFixed(3); };
const deviceDraw = headtrackr.ccv.drawFrames, hasDevice = typeof deviceDraw === 'function';
function force(canvas, device) { /* every 5-argument drawImage onto `canvas` goes the chosen way */
  const ctx = canvas.getContext('2d'), hostDraw = Object.getPrototypeOf(ctx).drawImage;
  let inside = false;
  headtrackr.ccv.drawFrames = function (v, c) { hostDraw.call(c.getContext('2d'), v, 0, 0, c.width, c.height); return c; };
  ctx.drawImage = !device ? hostDraw : function (v) {
    if (inside || arguments.length !== 5) return hostDraw.apply(this, arguments);
    inside = true;
    try { deviceDraw(v, canvas); } finally { inside = false; }
  };
}

function frame(w, h, k) {
  const px = new Uint8Array(w * h * 4).fill(110), s = h >> 1, x0 = (w >> 2) + 3 * k, y0 = (h >> 3) + 2 * k;
  for (let y = 0; y < s; y++) for (let x = 0; x < s; x++) { const p = ((y0 + y) * w + x0 + x) * 4, v = 60 + ((x * 7 + y * 13) & 127); px[p] = v; px[p + 1] = (3 * v) >> 2; px[p + 2] = (3 * v / 5) | 0; }
  for (let p = 3; p < px.length; p += 4) px[p] = 255;
  return px;
}

[[640, 480], [1280, 720], [1920, 1080]].forEach(function (sz) {
  const vw = sz[0], vh = sz[1], W = 320, H = 240, nf = 4;
  const frames = [], video = new Canvas(vw, vh);
  for (let k = 0; k < nf; k++) frames.push(frame(vw, vh, k));
  const run = function (device, blocks) {
    const canvas = new Canvas(W, H), t = [];
    const tr = new headtrackr.Tracker({ whitebalancing: false, calcAngles: true });
    force(canvas, device);
    let i = 0;
    tr.init(video, canvas);
    for (let b = 0; b < blocks; b++) {
      for (let k = 0; k < steps; k++, i++) {
        video.setFrame(frames[i % nf]); /* the camera delivers the next frame: not part of the step */
        const t0 = now();
        tr.step();
        if (b > 0) t.push(now() - t0);
      }
    }
    return t;
  };
  const host = [], dev = [];
  for (let r = 0; r < 3; r++) { /* alternate the routes */
    Array.prototype.push.apply(host, run(false, 2));
    if (hasDevice) Array.prototype.push.apply(dev, run(true, 2));
  }
  /* the draws alone */
  const canvas = new Canvas(W, H), dh = [], dd = [];
  for (let i = 0; i < steps + 5; i++) {
    video.setFrame(frames[i % nf]);
    let t0 = now();
    canvas.getContext('2d').drawImage(video, 0, 0, W, H);
    if (i >= 5) dh.push(now() - t0);
    if (hasDevice) { t0 = now(); deviceDraw(video, canvas); if (i >= 5) dd.push(now() - t0); }
  }
  console.log(JSON.stringify({ root: root, video: vw + 'x' + vh, canvas: W + 'x' + H, steps_per_route: host.length,
    step_ms_p50_host_draw: p50(host), step_ms_p50_device_draw: hasDevice ? p50(dev) : null,
    draw_ms_p50_host: p50(dh), draw_ms_p50_device: hasDevice ? p50(dd) : null }));
});
process.stdout.write('', function () { headtrackr.exitNow(0); });
